"""CPU: the device plonky3 prover's handle and argument rules in the C ABI (include/p25.h: p25_p3_prover_create,
p25_p3_prover_config, p25_p3_prove_batch[_dev], p25_p3_prover_sync).

The handle is host-only until its first compute call: creating it, asking its shape and every argument refusal work without
a GPU; the compute entry points then answer P25_ERR_NO_DEVICE.  What `create` accepts and refuses is what the host prover
p25_p3_prove_air_ex accepts and refuses for the same arguments."""
import ctypes as C

import numpy as np
import pytest

import air_cases
from conftest import P

OK, INVALID_ARG, NO_DEVICE = 0, 1, 2


def _gpu():
    import torch
    return torch.cuda.is_available()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _last(p25):
    return p25.lib().p25_last_error().decode()


def _create(p25, air, log_n, log_blowup, queries, pow_bits):
    ac, h = air.to_c(), C.c_void_p()
    st = p25.lib().p25_p3_prover_create(C.byref(ac), log_n, log_blowup, queries, pow_bits, C.byref(h))
    if st == OK:
        assert h.value
        p25.lib().p25_p3_prover_destroy(h)
    else:
        assert not h.value and _last(p25)
    return st


def _host(p25, air, trace, log_n, log_blowup, queries, pow_bits):
    """Status of the host prover for the same arguments (it proves: small shapes only)."""
    ac, n = air.to_c(), C.c_size_t(0)
    out = np.zeros(1 << 16, dtype=np.uint64)
    return p25.lib().p25_p3_prove_air_ex(C.byref(ac), _p(trace), log_n, log_blowup, queries, pow_bits, 0, 1, _p(out), out.size,
                                         C.byref(n), None)


# (log_n, queries, pow_bits): the table of tests/test_p3_prover.py::test_bad_parameters, then the other bounds
FIB_ARGS = [((0, 1, 10, 8), False), ((23, 1, 10, 8), False), ((5, 1, 0, 8), False), ((5, 1, 10, 8), True),
            ((3, 0, 3, 4), False), ((3, 5, 3, 4), False), ((3, 4, 3, 4), True), ((3, 1, 3, -1), False), ((3, 1, 3, 31), False),
            ((3, 1, 3, 30), True), ((3, 1, 3, 0), True), ((1, 1, 1, 0), True), ((22, 3, 3, 4), False), ((21, 4, 3, 4), False),
            ((22, 2, 3, 4), True), ((3, 1, -1, 4), False)]


@pytest.mark.parametrize("args,accepted", FIB_ARGS)
def test_create_accepts_what_the_host_prover_accepts(p25, args, accepted):
    log_n, log_blowup, queries, pow_bits = args
    air = p25.Air.fibonacci()
    st = _create(p25, air, log_n, log_blowup, queries, pow_bits)
    assert st == (OK if accepted else INVALID_ARG)
    if log_n <= 5:    # the host prover's verdict for the same arguments (it never reads the trace of a refused shape)
        trace = air_cases.fib_trace(max(log_n, 1))
        host = _host(p25, air, trace, log_n, log_blowup, queries, 0 if accepted and pow_bits > 8 else pow_bits)
        assert (host == OK) == accepted and host in (OK, INVALID_ARG)


def test_create_refuses_a_degree_the_blowup_cannot_hold(p25):
    air, par = air_cases.quartic_map(p25, 3)
    trace = air_cases.quartic_map_trace(par, 3)
    assert _create(p25, air, 3, 1, 3, 4) == INVALID_ARG
    assert _host(p25, air, trace, 3, 1, 3, 4) == INVALID_ARG
    assert _create(p25, air, 3, 2, 3, 4) == OK
    assert _host(p25, air, trace, 3, 2, 3, 4) == OK
    cub = air_cases.cubic(p25)
    assert _create(p25, cub, 3, 1, 3, 4) == OK


def test_create_refuses_null_and_malformed_airs(p25):
    lib, h = p25.lib(), C.c_void_p()
    ac = p25.Air.fibonacci().to_c()
    assert lib.p25_p3_prover_create(None, 3, 1, 3, 4, C.byref(h)) == INVALID_ARG and "null" in _last(p25)
    assert lib.p25_p3_prover_create(C.byref(ac), 3, 1, 3, 4, None) == INVALID_ARG and "null" in _last(p25)
    bad = p25.Air(2)
    bad.assert_zero(bad.sub(bad.local(0), bad.local(5)))    # a column the AIR does not have
    assert _create(p25, bad, 3, 1, 3, 4) == INVALID_ARG


def test_create_accepts_every_test_air_and_a_wide_one(p25):
    airs = [air_cases.tribonacci(p25), air_cases.squares(p25), air_cases.cubic(p25), air_cases.cubic_transition(p25),
            air_cases.quadratic_pair(p25, 1)[0], air_cases.quartic_map(p25, 1)[0], air_cases.quintic_selector(p25, 1)[0]]
    airs += [air_cases.random_recurrence(p25, 7, w)[0] for w in (2, 5, 9, 64)]
    for air in airs:
        assert _create(p25, air, 4, 2, 3, 4) == OK, _last(p25)
    # width 64, more than 512 nodes: every column squared, summed in a chain, pinned by one constraint per column
    wide = p25.Air(64)
    acc = wide.const(0)
    for j in range(64):
        x = wide.local(j)
        acc = wide.add(acc, wide.mul(x, x))
        wide.when_transition(wide.sub(wide.next(j), wide.add(wide.mul(wide.const(j + 2), x), acc)))
    assert len(wide.nodes) >= 512
    assert _create(p25, wide, 4, 1, 3, 4) == OK, _last(p25)


def test_create_names_the_live_value_limit(p25):
    """A DAG that needs more intermediate values at once than the device form holds is refused at create, by name."""
    air = p25.Air(2)
    x = air.local(0)
    powers = [air.mul(x, air.const(3))]
    for _ in range(80):
        powers.append(air.add(powers[-1], x))
    total = powers[0]
    for v in reversed(powers[1:]):      # the first value is used last: all 81 sums are alive together
        total = air.add(total, v)
    air.when_first_row(air.sub(total, air.local(1)))
    assert _create(p25, air, 3, 1, 3, 4) == INVALID_ARG
    assert "alive" in _last(p25) and "64" in _last(p25)


SHAPES = [("fib", 3, 1, 3, 4), ("fib", 6, 1, 100, 16), ("trib", 4, 1, 5, 0), ("cubic", 5, 1, 7, 3), ("quintic", 4, 2, 9, 5),
          ("fib", 3, 4, 2, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_config_equals_the_host_provers(p25, shape):
    name, log_n, log_blowup, queries, pow_bits = shape
    air = {"fib": p25.Air.fibonacci, "trib": lambda: air_cases.tribonacci(p25), "cubic": lambda: air_cases.cubic(p25),
           "quintic": lambda: air_cases.quintic_selector(p25, 2)[0]}[name]()
    pr = p25.P3Prover(air, log_n, log_blowup, queries, pow_bits)
    ac, n, cfg = air.to_c(), C.c_size_t(0), p25.P3Config()
    assert p25.lib().p25_p3_prove_air_ex(C.byref(ac), None, log_n, log_blowup, queries, pow_bits, 0, 1, None, 0, C.byref(n),
                                         C.byref(cfg)) == OK
    assert pr.num_inputs == n.value
    assert bytes(pr.config) == bytes(cfg)
    assert pr.config.log_quotient_degree == {"fib": 0, "trib": 0, "cubic": 1, "quintic": 2}[name]
    # both outputs are optional
    assert p25.lib().p25_p3_prover_config(pr._h, None, None) == OK
    pr.close()


@pytest.fixture(scope="module")
def fx(p25):
    pr = p25.P3Prover(p25.Air.fibonacci(), 3, 1, 3, 4)
    trace = air_cases.fib_trace(3)
    return pr, trace, np.zeros(pr.num_inputs, dtype=np.uint64), np.zeros(1, dtype=np.int32)


def test_null_handle_is_refused(p25, fx):
    lib = p25.lib()
    _pr, trace, out, st = fx
    n = C.c_size_t(0)
    for call in (lambda: lib.p25_p3_prover_config(None, None, C.byref(n)),
                 lambda: lib.p25_p3_prove_batch(None, _p(trace), 1, None, _p(out), out.size, _p(st)),
                 lambda: lib.p25_p3_prove_batch_dev(None, None, 24, 1, None, None, out.size, None, None),
                 lambda: lib.p25_p3_prover_sync(None)):
        assert call() == INVALID_ARG
        assert "null" in _last(p25)
    lib.p25_p3_prover_destroy(None)     # like free(NULL)


def test_argument_errors_come_before_the_device(p25, fx):
    lib = p25.lib()
    pr, trace, out, st = fx
    h, ni = pr._h, pr.num_inputs
    cases = {
        "null traces": lambda: lib.p25_p3_prove_batch(h, None, 1, None, _p(out), ni, _p(st)),
        "null outputs": lambda: lib.p25_p3_prove_batch(h, _p(trace), 1, None, None, ni, _p(st)),
        "null statuses": lambda: lib.p25_p3_prove_batch(h, _p(trace), 1, None, _p(out), ni, None),
        "short stride": lambda: lib.p25_p3_prove_batch(h, _p(trace), 1, None, _p(out), ni - 1, _p(st)),
        "dev null outputs": lambda: lib.p25_p3_prove_batch_dev(h, None, 24, 1, None, None, ni, None, None),
        "dev short stride": lambda: lib.p25_p3_prove_batch_dev(h, _p(trace), 24, 1, None, _p(out), ni - 1, _p(st), None),
        "dev short trace stride": lambda: lib.p25_p3_prove_batch_dev(h, _p(trace), 23, 1, None, _p(out), ni, _p(st), None),
    }
    for name, call in cases.items():
        assert call() == INVALID_ARG, name
        assert _last(p25), name
    assert "input_stride" in _last(p25) or "trace_stride" in _last(p25)


def test_host_form_refuses_non_canonical_words(p25, fx):
    lib = p25.lib()
    pr, trace, out, st = fx
    bad = trace.copy()
    bad[5, 1] = P
    out[:] = 77
    assert lib.p25_p3_prove_batch(pr._h, _p(bad), 1, None, _p(out), out.size, _p(st)) == INVALID_ARG
    assert "non-canonical" in _last(p25)
    start = np.array([P], dtype=np.uint64)
    assert lib.p25_p3_prove_batch(pr._h, _p(trace), 1, _p(start), _p(out), out.size, _p(st)) == INVALID_ARG
    assert "non-canonical" in _last(p25)
    assert (out == 77).all()     # nothing was launched, nothing written


def test_empty_batch_touches_nothing(p25, fx):
    lib = p25.lib()
    pr, _trace, _out, _st = fx
    assert lib.p25_p3_prove_batch(pr._h, None, 0, None, None, 0, None) == OK
    assert lib.p25_p3_prove_batch_dev(pr._h, None, 0, 0, None, None, 0, None, None) == OK


def test_compute_needs_a_device(p25, fx):
    lib = p25.lib()
    pr, trace, out, st = fx
    s = lib.p25_p3_prove_batch(pr._h, _p(trace), 1, None, _p(out), out.size, _p(st))
    if _gpu():
        assert s == OK and st[0] == OK
        want, _cfg = p25.p3_prove_air(p25.Air.fibonacci(), trace, num_queries=3, pow_bits=4, threads=1)
        assert np.array_equal(out, want)
        assert lib.p25_p3_prover_sync(pr._h) == OK
    else:
        assert s == NO_DEVICE and "no CPU fallback" in _last(p25)
        assert lib.p25_p3_prover_sync(pr._h) == NO_DEVICE
