"""CPU: the device plonky3 prover's handle and argument rules in the C ABI (include/p25.h: p25_p3_prover_create,
p25_p3_prover_config, p25_p3_prove_batch[_dev], p25_p3_prover_sync).

The handle is host-only until its first compute call: creating it, asking its shape and every argument refusal work without
a GPU; the compute entry points then answer P25_ERR_NO_DEVICE.  What `create` accepts and refuses is what the host prover
p25_p3_prove_air_ex accepts and refuses for the same arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import air_cases
from conftest import P, ROOT

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


def _prove_or_status(p25, air, trace, log_blowup):
    """The host prover's (words, OK) or (None, status) for a trace, with the arguments of the generated-AIR cases."""
    try:
        return p25.p3_prove_air(air, trace, num_queries=air_cases.DAG_QUERIES, pow_bits=air_cases.DAG_POW_BITS,
                                log_blowup=log_blowup)[0], OK
    except p25.P25Error as e:
        return None, e.status


def test_live_chain_boundary(p25):
    """air_cases.live_chain(m) keeps v0 .. v_m alive until the sum starts, and the sum's first node takes the slot that
    v0 or v_m gave back: m + 1 slots.  So the largest accepted m is P3_MAX_LIVE - 1, the accepted program uses every slot
    index, and one more value is refused by name.  The figure is measured, not written down: a change of the allocator
    that moves it fails here and has to state the new relation."""
    hdr = open(os.path.join(ROOT, "plonky2.5_amd", "csrc", "p3_kernels.h")).read()
    max_live = int(re.search(r"constexpr\s+uint32_t\s+P3_MAX_LIVE\s*=\s*(\d+)\s*;", hdr).group(1))
    accepted = [m for m in range(1, 2 * max_live) if _create(p25, air_cases.live_chain(p25, m), 3, 1, 3, 4) == OK]
    assert accepted and accepted == list(range(1, accepted[-1] + 1))      # one boundary, nothing accepted beyond it
    m = accepted[-1]
    assert m == max_live - 1
    assert _create(p25, air_cases.live_chain(p25, m + 1), 3, 1, 3, 4) == INVALID_ARG
    assert "alive" in _last(p25) and f"keeps {max_live + 1} " in _last(p25) and f"at most {max_live}" in _last(p25)
    # the chains on both sides of the boundary are valid inputs: the host prover, which has no such limit, proves them
    for mm in (m, m + 1):
        assert _prove_or_status(p25, air_cases.live_chain(p25, mm), air_cases.live_chain_trace(mm, 3), 1)[1] == OK


def test_slots_go_back_on_last_use(p25):
    """air_cases.slot_churn has far more arithmetic nodes than P3_MAX_LIVE and a handful alive at a time; more than
    P3_MAX_LIVE of them end their life as a left operand, as a right operand and as a constraint's root.  A compile that
    forgets to give back any of the three runs out of slots and refuses it; the live chain cannot see that, since a slot
    leaked there is a slot the chain no longer needs."""
    air, y = air_cases.slot_churn(p25)
    arith = [nd for nd in air.nodes if nd[0] >= 3]
    is_arith = lambda i: air.nodes[i][0] >= 3
    assert sum(is_arith(nd[1]) for nd in arith) > 2 * 64 and sum(is_arith(nd[2]) for nd in arith) > 2 * 64
    assert sum(is_arith(c) for c, _w in air.constraints) > 64
    assert _create(p25, air, 3, 1, 3, 4) == OK, _last(p25)
    assert _prove_or_status(p25, air, air_cases.slot_churn_trace(air, y, 3), 1)[1] == OK


def test_random_dag_cases_are_valid_and_mix_verdicts(p25):
    """The 48 generated cases of tests/test_gpu_p3_prover_forms.py, on the host alone: every one is created (so none
    passes P3_MAX_LIVE), the host prover accepts its trace, and the trace with DAG_BAD_CELL incremented is refused in at
    least 12 cases and accepted in at least 6 (the cell is free where its constraint is not enforced)."""
    refused = accepted = 0
    for max_degree, log_blowup in air_cases.DAG_CLASSES:
        for seed in air_cases.DAG_SEEDS:
            air, trace = air_cases.dag_case(p25, seed, max_degree)
            assert trace.shape == (1 << air_cases.DAG_LOG_N, 16) and (trace < P).all()
            assert len(air.constraints) == 10 and len(air.nodes) > 160
            assert _create(p25, air, air_cases.DAG_LOG_N, log_blowup, air_cases.DAG_QUERIES, air_cases.DAG_POW_BITS) == OK, \
                (seed, max_degree, _last(p25))
            assert _prove_or_status(p25, air, trace, log_blowup)[1] == OK, (seed, max_degree)
            st = _prove_or_status(p25, air, air_cases.bump(trace, *air_cases.DAG_BAD_CELL), log_blowup)[1]
            assert st in (OK, INVALID_ARG)
            refused += st == INVALID_ARG
            accepted += st == OK
    assert refused >= 12 and accepted >= 6, (refused, accepted)


def test_random_dag_shares_what_it_claims(p25):
    """The properties the generated DAGs are there for, counted over the 48 cases: a node read by several later nodes, a
    root shared by two constraints, a root that a later node reads again, the same operand twice in one node."""
    multi_use = shared_root = root_read_later = twice = 0
    for max_degree, _b in air_cases.DAG_CLASSES:
        for seed in air_cases.DAG_SEEDS:
            air, _t = air_cases.dag_case(p25, seed, max_degree)
            roots = [air.nodes[c][1] for c, _w in air.constraints]          # constraint = sub(root, local): operand a
            arith = {i for i, nd in enumerate(air.nodes) if nd[0] >= 3}
            reads = [x for i in arith for x in air.nodes[i][1:3] if x in arith]
            multi_use += any(reads.count(x) >= 3 for x in set(reads))
            shared_root += len(set(roots)) < len(roots)
            root_read_later += any(sum(1 for i in arith if i > r and r in air.nodes[i][1:3]) >= 2 for r in roots)
            twice += any(air.nodes[i][1] == air.nodes[i][2] and air.nodes[i][1] in arith for i in arith)
    assert min(multi_use, root_read_later, twice) >= 24 and shared_root >= 12, (multi_use, shared_root, root_read_later, twice)


def test_constant_and_single_cell_inputs(p25):
    """Inputs of the verdict tests of the GPU module, on the host alone: both constant traces are accepted and the first
    gives a proof full of zeros; of the 24 single-cell increments of an 8-row `squares` trace the host accepts exactly the
    free ones: y on the rows before the last."""
    for y0 in (0, 1):
        words = p25.p3_prove_air(air_cases.constant_pair(p25, y0), air_cases.constant_pair_trace(y0, 5), num_queries=3,
                                 pow_bits=4)[0]
        if y0 == 0:
            # zero by construction: the quotient's opening at zeta (2 words) and its value at every query (3 x 2), the
            # sibling value of 5 FRI rounds per query (3 x 5 x 2), the final polynomial (2)
            assert np.count_nonzero(words == 0) >= 2 + 6 + 30 + 2
    air, trace = air_cases.squares(p25), air_cases.squares_trace(3)
    ok_cells = []
    for r in range(8):
        for c in range(3):
            try:
                p25.p3_prove_air(air, air_cases.bump(trace, r, c), num_queries=3, pow_bits=4)
                ok_cells.append((r, c))
            except p25.P25Error as e:
                assert e.status == INVALID_ARG
    assert ok_cells == [(r, 2) for r in range(7)]


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
