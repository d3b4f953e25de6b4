"""CPU: periodic columns of the inner STARK (include/p25.h, "PERIODIC COLUMNS") -- the AIR form, the host prover, the
verifier-circuit builder.

A column of period P = 2^k is part of the AIR; node op 7 PERIODIC reads it at the current row.  It is neither committed nor
opened: the prover reads a coset table, every verifier evaluates it at zeta.  Expected verdicts come from the independent
model tests/p3_periodic_model.py (Lagrange form at zeta); the outer circuit is judged by the oracle, loaded from the exported
blob.  Every comparison is equality.

The mimc(k, d) cases run at the log_blowup their degree needs: the transition constraint next0 = (local0 + PERIODIC(0))^d has
degree d + 1 with its selector, so d = 2 / 3 / 5 take two / four / eight quotient chunks (log_blowup 1 / 2 / 3)."""
import ctypes as C

import numpy as np
import pytest

import air_cases_periodic as cases
import p3_periodic_model as M
from conftest import P

OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4


class Periodic(C.Structure):
    """p25_air_periodic, stated from the header."""
    _fields_ = [("n_columns", C.c_uint32), ("log_period", C.POINTER(C.c_uint32)), ("values", C.POINTER(C.c_uint64))]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _last(p25):
    return p25.lib().p25_last_error().decode()


def _prove(p25, air, trace, pv, log_blowup, queries=3, pow_bits=4):
    return p25.p3_prove_air(air, trace, num_queries=queries, pow_bits=pow_bits, log_blowup=log_blowup, threads=1,
                            public_values=pv)


def _changed(columns, c, j):
    out = [np.array(col, dtype=np.uint64) for col in columns]
    out[c][j] = (int(out[c][j]) + 1) % P
    return out


# ---- 1, 2. the host prover against the model ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_host_prover_words_pass_the_model(p25, oracle, shape):
    air, trace, pv, log_n, log_blowup = cases.make(p25, shape)
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    assert cfg.log_trace_height == log_n
    assert inp.size == M.Shape(cfg).num_inputs + air.n_public                  # the proof's layout does not change
    assert M.verify(oracle, air, cfg, inp) == M.OK
    # one value of one column changed: the identity fails, and nothing before it
    cols = air.periodic_columns
    for c, j in sorted({(0, 0), (len(cols) - 1, cols[-1].size - 1), (len(cols) // 2, cols[len(cols) // 2].size // 2)}):
        assert M.verify(oracle, air, cfg, inp, columns=_changed(cols, c, j)) == M.CONSTRAINTS, (c, j)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_a_changed_trace_cell_is_refused(p25, shape):
    air, trace, pv, log_n, log_blowup = cases.make(p25, shape)
    for r in sorted({0, (1 << log_n) - 1, (1 << log_n) // 2}):
        bad = trace.copy()
        bad[r, trace.shape[1] - 1] = (int(bad[r, trace.shape[1] - 1]) + 1) % P
        with pytest.raises(p25.P25Error) as ei:
            _prove(p25, air, bad, pv, log_blowup)
        assert ei.value.status == INVALID_ARG, r


# ---- 3. n_columns = 0 is the form without columns -------------------------------------------------------------------
def test_no_columns_reproduce_the_words_and_the_blob(p25):
    from air_cases_pv import fib_pv, fib_pv_trace
    lib = p25.lib()
    air = fib_pv(p25)
    trace, pv = fib_pv_trace(4, 2, 3)
    want, cfg = p25.p3_prove_air(air, trace, num_queries=4, pow_bits=5, log_blowup=2, threads=1, public_values=pv)
    ac = air.to_c()
    empty = Periodic(0, None, None)
    for periodic in (None, C.byref(empty)):
        n, c2 = C.c_size_t(0), p25.P3Config()
        assert lib.p25_p3_prove_air_pc(C.byref(ac), _p(trace), _p(pv), periodic, 4, 2, 4, 5, 0, 1, None, 0, C.byref(n),
                                       C.byref(c2)) == OK
        assert n.value == want.size                                            # the size query
        out = np.zeros(n.value, dtype=np.uint64)
        assert lib.p25_p3_prove_air_pc(C.byref(ac), _p(trace), _p(pv), periodic, 4, 2, 4, 5, 0, 1, _p(out), out.size,
                                       C.byref(n), C.byref(c2)) == OK, _last(p25)
        assert (out == want).all() and bytes(c2) == bytes(cfg)
        # the circuit: byte for byte the blob of p25_circuit_build_p3_verifier_air
        h = C.c_void_p()
        assert lib.p25_circuit_build_p3_verifier_air_pc(C.byref(cfg), C.byref(ac), periodic, C.byref(h)) == OK, _last(p25)
        blob = p25.Circuit(h.value).to_blob()
        assert blob == p25.Circuit.build_p3_verifier_air(cfg, air).to_blob()
        # the handle: the same shape, the same num_inputs
        h = C.c_void_p()
        assert lib.p25_p3_prover_create_pc(C.byref(ac), periodic, 4, 2, 4, 5, C.byref(h)) == OK, _last(p25)
        c3, n3 = p25.P3Config(), C.c_size_t(0)
        assert lib.p25_p3_prover_config(h, C.byref(c3), C.byref(n3)) == OK
        lib.p25_p3_prover_destroy(h)
        assert bytes(c3) == bytes(cfg) and n3.value == want.size


# ---- 4. validation --------------------------------------------------------------------------------------------------
def _entry_points(p25, air, log_n, columns):
    """The three _pc entry points on `air` with `columns` (raw: a list of (log_period, values) that need not agree) ->
    [(status, message)]; nothing may be written."""
    lib = p25.lib()
    ac = air.to_c()
    lp = (C.c_uint32 * max(1, len(columns)))(*[k for k, _ in columns])
    flat = [int(v) for _, vals in columns for v in vals]
    vals = (C.c_uint64 * max(1, len(flat)))(*flat)
    pc = Periodic(len(columns), lp, vals)
    trace = np.zeros((1 << log_n, air.width), dtype=np.uint64)
    out = np.zeros(1 << 14, dtype=np.uint64)
    res = []
    n = C.c_size_t(12345)
    st = lib.p25_p3_prove_air_pc(C.byref(ac), _p(trace), None, C.byref(pc), log_n, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n),
                                 None)
    res.append((st, _last(p25)))
    assert n.value == 12345 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create_pc(C.byref(ac), C.byref(pc), log_n, 1, 3, 4, C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    cfg = p25.P3Config(1, 3, 4, 0, log_n, air.width, log_n + 1, 2, log_n)
    st = lib.p25_circuit_build_p3_verifier_air_pc(C.byref(cfg), C.byref(ac), C.byref(pc), C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    return res


def _reads_column(p25, index):
    air = p25.Air(2)
    air.assert_zero(air.sub(air.local(1), air.mul(air.local(0), air.periodic(index))))
    return air


@pytest.mark.parametrize("name,index,log_n,columns,word", [
    ("index = n_columns", 1, 3, [(1, [1, 2])], "n_columns"),
    ("no columns at all", 0, 3, [], "n_columns"),
    ("log_period 0", 0, 3, [(0, [1])], "log_period"),
    ("log_period 9", 0, 10, [(9, [1] * 512)], "P25_AIR_MAX_LOG_PERIOD"),
    ("log_period above log_n", 0, 2, [(3, [1] * 8)], "log_n"),
    ("a value = p", 0, 3, [(2, [1, 2, P, 4])], ">= p"),
    ("33 columns", 0, 3, [(1, [1, 2])] * 33, "P25_AIR_MAX_PERIODIC"),
])
def test_validation_names_the_limit(p25, name, index, log_n, columns, word):
    for st, msg in _entry_points(p25, _reads_column(p25, index), log_n, columns):
        assert st == INVALID_ARG and word in msg, (name, st, msg)


def test_the_caps_themselves_are_accepted(p25):
    """32 columns of period 256 at log_n 8: the handle and the circuit builder take them."""
    air = cases.per_mix(p25, [8] * 32)
    pr = p25.P3Prover(air, 8, 1, 3, 4)
    assert pr.config.log_quotient_degree == 0
    c = p25.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(c.info.num_inputs) == pr.num_inputs


def test_the_forms_without_columns_refuse_op_7_and_write_nothing(p25):
    lib = p25.lib()
    air = _reads_column(p25, 0)                                                # the binding would take the _pc route: raw calls
    ac = air.to_c()
    trace = np.zeros((8, 2), dtype=np.uint64)
    out = np.zeros(4096, dtype=np.uint64)
    n = C.c_size_t(777)
    st = lib.p25_p3_prove_air(C.byref(ac), _p(trace), 3, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pc" in _last(p25)
    st = lib.p25_p3_prove_air_ex(C.byref(ac), _p(trace), 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pc" in _last(p25)
    st = lib.p25_p3_prove_air_pv(C.byref(ac), _p(trace), None, 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pc" in _last(p25)
    assert n.value == 777 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create(C.byref(ac), 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_pc" in _last(p25) and not h.value
    cfg = p25.P3Config(1, 3, 4, 0, 3, 2, 4, 2, 3)
    st = lib.p25_circuit_build_p3_verifier_air(C.byref(cfg), C.byref(ac), C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_pc" in _last(p25) and not h.value


# ---- 5. degree ------------------------------------------------------------------------------------------------------
def test_periodic_counts_as_degree_one(p25):
    air = p25.Air(2, periodic=[np.array([3, 4], dtype=np.uint64)])
    x = air.local(0)
    air.assert_zero(air.sub(air.mul(air.periodic(0), air.mul(x, x)), air.local(1)))    # PERIODIC * LOCAL * LOCAL: degree 3
    pr = p25.P3Prover(air, 3, 1, 3, 4)
    assert pr.config.log_quotient_degree == 1
    assert p25.P3Prover(cases.mimc(p25, 2, 2), 3, 1, 3, 4).config.log_quotient_degree == 1
    assert p25.P3Prover(cases.mimc(p25, 2, 3), 3, 2, 3, 4).config.log_quotient_degree == 2
    assert p25.P3Prover(cases.mimc(p25, 2, 5), 3, 3, 3, 4).config.log_quotient_degree == 3


@pytest.mark.parametrize("d", [3, 5])
def test_more_chunks_than_log_blowup_holds_is_refused(p25, d):
    """mimc(2, 3) needs four chunks, mimc(2, 5) eight: neither fits log_blowup 1."""
    air = cases.mimc(p25, 2, d)
    trace, pv = cases.mimc_trace(3, 2, d, 3)
    with pytest.raises(p25.P25Error) as ei:
        _prove(p25, air, trace, pv, 1)
    assert ei.value.status == INVALID_ARG and "log_blowup" in str(ei.value)
    with pytest.raises(p25.P25Error) as ei:
        p25.P3Prover(air, 3, 1, 3, 4)
    assert ei.value.status == INVALID_ARG and "chunks" in str(ei.value)


# ---- 6. the verifier circuit ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mimc_outer(p25, oracle):
    air = cases.mimc(p25, 2, 3)
    trace, pv = cases.mimc_trace(3, 2, 3, 11)
    inp, cfg = _prove(p25, air, trace, pv, 2)
    c = p25.Circuit.build_p3_verifier_air(cfg, air)
    return air, cfg, inp, pv, c, oracle.load_circuit(c.to_blob())


def test_oracle_proves_and_verifies_the_outer_circuit(mimc_outer):
    air, cfg, inp, pv, c, oc = mimc_outer
    wires, st, msg = oc.witness(inp, seed=3)
    assert st == 0, msg
    bad, msg = oc.check_constraints(wires)
    assert bad == 0, msg
    proof, st, _tm, msg = oc.prove(inp, seed=3)
    assert st == 0, msg
    assert proof[-2:].tolist() == [int(v) for v in pv]
    assert oc.verify(proof)[0] == 0


@pytest.mark.parametrize("j", [0, 3])
def test_a_changed_round_constant_is_a_witness_conflict(p25, oracle, mimc_outer, j):
    """The circuit's coefficient / Horner path against the prover's table path: the same inner proof, a circuit built with
    one round constant changed."""
    air, cfg, inp, pv, c, oc = mimc_outer
    rc = cases.mimc_constants(2).copy()
    rc[j] = (int(rc[j]) + 1) % P
    other = p25.Circuit.build_p3_verifier_air(cfg, cases.mimc(p25, 2, 3, constants=rc))
    assert other.to_blob() != c.to_blob()
    assert oracle.load_circuit(other.to_blob()).witness(inp, seed=3)[1] == WITNESS_CONFLICT
