"""CPU: preprocessed columns of the inner STARK (include/p25.h, "PREPROCESSED COLUMNS") -- the AIR form, the host prover, the
commitment, the verifier-circuit builder.

A preprocessed matrix is committed once; its commitment is verifying-key data.  Node ops 8 PREP_LOCAL / 9 PREP_NEXT read it
at the current / next row.  A proof opens it at zeta and zeta w_n behind the chunk openings and carries a third batch per
query.  Expected verdicts come from the independent model tests/p3_preprocessed_model.py, which takes the commitment as an
argument and reaches it through the Merkle paths only; the commitment itself is compared with the model's statement of its
definition; the outer circuit is judged by the oracle, loaded from the exported blob.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import air_cases_preprocessed as cases
import p3_preprocessed_model as M
from conftest import P

OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4


class Preprocessed(C.Structure):
    """p25_air_preprocessed, stated from the header."""
    _fields_ = [("width", C.c_uint32), ("log_n", C.c_uint32), ("values", C.POINTER(C.c_uint64))]


class Periodic(C.Structure):
    _fields_ = [("n_columns", C.c_uint32), ("log_period", C.POINTER(C.c_uint32)), ("values", C.POINTER(C.c_uint64))]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _last(p25):
    return p25.lib().p25_last_error().decode()


def _prove(p25, air, trace, pv, log_blowup, queries=3, pow_bits=4):
    return p25.p3_prove_air(air, trace, num_queries=queries, pow_bits=pow_bits, log_blowup=log_blowup, threads=1,
                            public_values=pv)


def _raw(prep):
    """(p25_air_preprocessed, keep-alive) of a matrix, without the binding's checks."""
    a = np.ascontiguousarray(prep, dtype=np.uint64)
    return Preprocessed(a.shape[1], int(a.shape[0]).bit_length() - 1, a.ctypes.data_as(C.POINTER(C.c_uint64))), a


# ---- 1. the host prover against the model; 10. num_inputs ------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_host_prover_words_pass_the_model(p25, oracle, shape):
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, shape)
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    assert cfg.log_trace_height == log_n
    pw = prep.shape[1]
    assert inp.size == M.num_inputs_formula(cfg, pw, air.n_public) == M.Shape(cfg, pw).num_inputs + air.n_public
    commit = p25.p3_preprocessed_commit(prep, log_blowup, threads=1)
    assert M.verify(oracle, air, cfg, inp, commit) == M.OK
    # another key: the transcript parts ways with the prover's at the first challenge
    other = commit.copy()
    other[3] = (int(other[3]) + 1) % P
    assert M.verify(oracle, air, cfg, inp, other) != M.OK


@pytest.mark.parametrize("name", ["mix1", "mix5", "mix9", "machine2", "mix2_b4"])
def test_the_commitment_is_the_models(p25, oracle, name):
    """p25_p3_preprocessed_commit against the definition: Lagrange interpolation, point-by-point evaluation on the coset,
    the MMCS over bit-reversed leaves."""
    _air, _trace, _pv, prep, _log_n, log_blowup = cases.make(p25, cases.shape(name))
    assert p25.p3_preprocessed_commit(prep, log_blowup, threads=1).tolist() == M.model_commit(oracle, prep, log_blowup)


def test_num_inputs_is_the_formula_on_every_route(p25):
    """The size query, the handle and the circuit agree with the formula, public values included."""
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, cases.shape("machine2_per"))
    lib = p25.lib()
    ac, pc = air.to_c(), air.periodic_to_c()
    pp, _keep = _raw(prep)
    n, cfg = C.c_size_t(0), p25.P3Config()
    assert lib.p25_p3_prove_air_pp(C.byref(ac), None, None, C.byref(pc), C.byref(pp), log_n, log_blowup, 5, 4, 0, 1, None, 0,
                                   C.byref(n), C.byref(cfg)) == OK, _last(p25)
    want = M.num_inputs_formula(cfg, 2, 2)
    assert n.value == want
    pr = p25.P3Prover(air, log_n, log_blowup, 5, 4)
    assert pr.num_inputs == want and bytes(pr.config) == bytes(cfg)
    assert int(p25.Circuit.build_p3_verifier_air(cfg, air).info.num_inputs) == want


# ---- 2, 3. what the prover refuses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_a_changed_trace_cell_is_refused(p25, shape):
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, shape)
    for r in sorted({0, (1 << log_n) - 1, (1 << log_n) // 2}):
        bad = trace.copy()
        bad[r, trace.shape[1] - 1] = (int(bad[r, trace.shape[1] - 1]) + 1) % P
        with pytest.raises(p25.P25Error) as ei:
            _prove(p25, air, bad, pv, log_blowup)
        assert ei.value.status == INVALID_ARG and "quotient identity" in str(ei.value), r


@pytest.mark.parametrize("name", ["mix9", "machine2", "machine3", "machine2_per"])
def test_a_changed_preprocessed_cell_on_the_provers_side_is_refused(p25, oracle, name):
    """The trace was made under the shape's columns: under columns that differ in one cell it does not satisfy the AIR --
    unless it is recomputed, and then the proof is one under ANOTHER key."""
    shp = cases.shape(name)
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, shp)
    for r, c in sorted({(0, 0), ((1 << log_n) - 2, prep.shape[1] - 1), ((1 << log_n) // 2, prep.shape[1] // 2)}):
        other = prep.copy()
        other[r, c] = (int(other[r, c]) + 1) % P if shp[1] == "mix" or c else int(other[r, c]) ^ 1
        air2, trace2, pv2, _prep, _k, _b = cases.make(p25, shp, prep=other)
        with pytest.raises(p25.P25Error) as ei:
            _prove(p25, air2, trace, pv, log_blowup)
        assert ei.value.status == INVALID_ARG and "quotient identity" in str(ei.value), (r, c)
        inp, cfg = _prove(p25, air2, trace2, pv2, log_blowup)
        key, key2 = (p25.p3_preprocessed_commit(m, log_blowup, threads=1) for m in (prep, other))
        assert key.tolist() != key2.tolist()
        assert M.verify(oracle, air2, cfg, inp, key2) == M.OK
        assert M.verify(oracle, air, cfg, inp, key) != M.OK


# ---- 4. no columns: the _pc functions, byte for byte ------------------------------------------------------------------
def test_no_columns_reproduce_the_pc_words_and_the_blob(p25):
    import air_cases_periodic as per
    lib = p25.lib()
    air = per.mimc(p25, 2, 2)
    trace, pv = per.mimc_trace(3, 2, 2, 9)
    want, cfg = p25.p3_prove_air(air, trace, num_queries=4, pow_bits=5, log_blowup=1, threads=1, public_values=pv)
    want_blob = p25.Circuit.build_p3_verifier_air(cfg, air).to_blob()
    ac, pc = air.to_c(), air.periodic_to_c()
    dummy = np.zeros(1, dtype=np.uint64)
    empty = Preprocessed(0, 0, None)
    empty_with_garbage = Preprocessed(0, 17, dummy.ctypes.data_as(C.POINTER(C.c_uint64)))
    for prep in (None, C.byref(empty), C.byref(empty_with_garbage)):
        n, c2 = C.c_size_t(0), p25.P3Config()
        assert lib.p25_p3_prove_air_pp(C.byref(ac), _p(trace), _p(pv), C.byref(pc), prep, 3, 1, 4, 5, 0, 1, None, 0, C.byref(n),
                                       C.byref(c2)) == OK
        assert n.value == want.size                                            # the size query
        out = np.zeros(n.value, dtype=np.uint64)
        assert lib.p25_p3_prove_air_pp(C.byref(ac), _p(trace), _p(pv), C.byref(pc), prep, 3, 1, 4, 5, 0, 1, _p(out), out.size,
                                       C.byref(n), C.byref(c2)) == OK, _last(p25)
        assert (out == want).all() and bytes(c2) == bytes(cfg)
        h = C.c_void_p()
        assert lib.p25_circuit_build_p3_verifier_air_pp(C.byref(cfg), C.byref(ac), C.byref(pc), prep, C.byref(h)) == OK, _last(p25)
        assert p25.Circuit(h.value).to_blob() == want_blob
        h = C.c_void_p()
        assert lib.p25_p3_prover_create_pp(C.byref(ac), C.byref(pc), prep, 3, 1, 4, 5, C.byref(h)) == OK, _last(p25)
        c3, n3 = p25.P3Config(), C.c_size_t(0)
        assert lib.p25_p3_prover_config(h, C.byref(c3), C.byref(n3)) == OK
        root = np.zeros(4, dtype=np.uint64)
        st = lib.p25_p3_prover_preprocessed_commit(h, _p(root))                # no columns: nothing to return
        lib.p25_p3_prover_destroy(h)
        assert bytes(c3) == bytes(cfg) and n3.value == want.size
        assert st == INVALID_ARG and "no preprocessed columns" in _last(p25) and not root.any()
    # ... and with neither kind of column, the plain functions'
    from air_cases_pv import fib_pv, fib_pv_trace
    air = fib_pv(p25)
    trace, pv = fib_pv_trace(4, 2, 3)
    want, cfg = p25.p3_prove_air(air, trace, num_queries=4, pow_bits=5, log_blowup=2, threads=1, public_values=pv)
    ac = air.to_c()
    out, n, c2 = np.zeros(want.size, dtype=np.uint64), C.c_size_t(0), p25.P3Config()
    assert lib.p25_p3_prove_air_pp(C.byref(ac), _p(trace), _p(pv), None, None, 4, 2, 4, 5, 0, 1, _p(out), out.size, C.byref(n),
                                   C.byref(c2)) == OK, _last(p25)
    assert (out == want).all() and bytes(c2) == bytes(cfg)
    h = C.c_void_p()
    assert lib.p25_circuit_build_p3_verifier_air_pp(C.byref(cfg), C.byref(ac), None, None, C.byref(h)) == OK, _last(p25)
    assert p25.Circuit(h.value).to_blob() == p25.Circuit.build_p3_verifier_air(cfg, air).to_blob()


# ---- 5. validation ---------------------------------------------------------------------------------------------------
def _entry_points(p25, air, log_n, width, prep_log_n, values):
    """The three _pp entry points on `air` with a raw p25_air_preprocessed -> [(status, message)]; nothing may be written."""
    lib = p25.lib()
    ac = air.to_c()
    vals = (C.c_uint64 * max(1, len(values)))(*[int(v) for v in values])
    pp = Preprocessed(width, prep_log_n, vals)
    trace = np.zeros((1 << log_n, air.width), dtype=np.uint64)
    out = np.zeros(1 << 14, dtype=np.uint64)
    res = []
    n = C.c_size_t(12345)
    st = lib.p25_p3_prove_air_pp(C.byref(ac), _p(trace), None, None, C.byref(pp), log_n, 1, 3, 4, 0, 1, _p(out), out.size,
                                 C.byref(n), None)
    res.append((st, _last(p25)))
    assert n.value == 12345 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create_pp(C.byref(ac), None, C.byref(pp), log_n, 1, 3, 4, C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    cfg = p25.P3Config(1, 3, 4, 0, log_n, air.width, log_n + 1, 2, log_n)
    st = lib.p25_circuit_build_p3_verifier_air_pp(C.byref(cfg), C.byref(ac), None, C.byref(pp), C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    return res


def _reads_column(p25, index, op=8):
    air = p25.Air(2)
    col = air.prep_local(index) if op == 8 else air.prep_next(index)
    air.assert_zero(air.sub(air.local(1), air.mul(air.local(0), col)))
    return air


@pytest.mark.parametrize("name,op,index,log_n,width,prep_log_n,values,word", [
    ("PREP_LOCAL index = width", 8, 2, 3, 2, 3, [1] * 16, "width"),
    ("PREP_NEXT index = width", 9, 1, 3, 1, 3, [1] * 8, "width"),
    ("no columns at all", 8, 0, 3, 0, 3, [], "width"),
    ("65 columns", 8, 0, 1, 65, 1, [1] * 130, "P25_AIR_MAX_PREPROCESSED"),
    ("log_n below the trace's", 8, 0, 3, 1, 2, [1] * 4, "log_n"),
    ("log_n above the trace's", 9, 0, 3, 1, 4, [1] * 16, "log_n"),
    ("a value = p", 8, 0, 2, 2, 2, [1, 2, 3, P, 5, 6, 7, 8], ">= p"),
])
def test_validation_names_the_limit(p25, name, op, index, log_n, width, prep_log_n, values, word):
    for st, msg in _entry_points(p25, _reads_column(p25, index, op), log_n, width, prep_log_n, values):
        assert st == INVALID_ARG and word in msg, (name, st, msg)


def test_the_commit_function_validates(p25):
    lib = p25.lib()
    out = np.zeros(4, dtype=np.uint64)
    vals = (C.c_uint64 * 130)(*([1] * 130))
    for pp, blowup, word in ((Preprocessed(65, 1, vals), 1, "P25_AIR_MAX_PREPROCESSED"), (Preprocessed(0, 3, vals), 1, "width"),
                             (Preprocessed(2, 3, vals), 5, "log_blowup"), (Preprocessed(2, 0, vals), 1, "log_n")):
        assert lib.p25_p3_preprocessed_commit(C.byref(pp), blowup, 1, _p(out)) == INVALID_ARG and word in _last(p25), word
    bad = (C.c_uint64 * 4)(1, 2, P, 4)
    assert lib.p25_p3_preprocessed_commit(C.byref(Preprocessed(2, 1, bad)), 1, 1, _p(out)) == INVALID_ARG and ">= p" in _last(p25)
    assert not out.any()


# ---- 6. the caps -------------------------------------------------------------------------------------------------------
def test_the_caps_themselves_are_accepted(p25):
    """64 columns: the host prover's words, the handle and the circuit builder take them, and agree on the size."""
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, cases.shape("mix64"))
    pr = p25.P3Prover(air, log_n, log_blowup, 3, 4)
    assert pr.config.log_quotient_degree == 1
    c = p25.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(c.info.num_inputs) == pr.num_inputs == M.num_inputs_formula(pr.config, 64, 0)


# ---- 7. the forms without columns ------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [8, 9])
def test_the_forms_without_columns_refuse_the_ops_and_write_nothing(p25, op):
    lib = p25.lib()
    air = _reads_column(p25, 0, op)                                            # no columns in the binding's Air: raw calls
    ac = air.to_c()
    trace = np.zeros((8, 2), dtype=np.uint64)
    out = np.zeros(4096, dtype=np.uint64)
    n = C.c_size_t(777)
    empty = Periodic(0, None, None)
    st = lib.p25_p3_prove_air(C.byref(ac), _p(trace), 3, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pp" in _last(p25)
    st = lib.p25_p3_prove_air_ex(C.byref(ac), _p(trace), 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pp" in _last(p25)
    st = lib.p25_p3_prove_air_pv(C.byref(ac), _p(trace), None, 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pp" in _last(p25)
    st = lib.p25_p3_prove_air_pc(C.byref(ac), _p(trace), None, C.byref(empty), 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pp" in _last(p25)
    assert n.value == 777 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create(C.byref(ac), 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_pp" in _last(p25) and not h.value
    st = lib.p25_p3_prover_create_pc(C.byref(ac), C.byref(empty), 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_pp" in _last(p25) and not h.value
    cfg = p25.P3Config(1, 3, 4, 0, 3, 2, 4, 2, 3)
    st = lib.p25_circuit_build_p3_verifier_air(C.byref(cfg), C.byref(ac), C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_pp" in _last(p25) and not h.value
    st = lib.p25_circuit_build_p3_verifier_air_pc(C.byref(cfg), C.byref(ac), C.byref(empty), C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_pp" in _last(p25) and not h.value


# ---- 8, 9. degree ------------------------------------------------------------------------------------------------------
def test_prep_ops_count_as_degree_one(p25):
    prep = cases.columns(3, 2)
    for col in ("prep_local", "prep_next"):
        air = p25.Air(2, preprocessed=prep)
        x = air.local(0)
        air.assert_zero(air.sub(air.mul(getattr(air, col)(1), air.mul(x, x)), air.local(1)))   # PREP * LOCAL * LOCAL: degree 3
        assert p25.P3Prover(air, 3, 1, 3, 4).config.log_quotient_degree == 1
        air = p25.Air(2, preprocessed=prep)
        air.assert_zero(air.sub(air.mul(getattr(air, col)(0), air.local(0)), air.local(1)))    # degree 2: one chunk
        assert p25.P3Prover(air, 3, 1, 3, 4).config.log_quotient_degree == 0
    m = cases.machine_columns(3)
    assert p25.P3Prover(cases.prep_machine(p25, 2, m), 3, 1, 3, 4).config.log_quotient_degree == 1
    assert p25.P3Prover(cases.prep_machine(p25, 3, m), 3, 2, 3, 4).config.log_quotient_degree == 2


def test_more_chunks_than_log_blowup_holds_is_refused(p25):
    """prep_machine(3) needs four chunks: they do not fit log_blowup 1."""
    m = cases.machine_columns(3)
    air = cases.prep_machine(p25, 3, m)
    trace, pv = cases.prep_machine_trace(3, m, 3)
    with pytest.raises(p25.P25Error) as ei:
        _prove(p25, air, trace, pv, 1)
    assert ei.value.status == INVALID_ARG and "log_blowup" in str(ei.value)
    with pytest.raises(p25.P25Error) as ei:
        p25.P3Prover(air, 3, 1, 3, 4)
    assert ei.value.status == INVALID_ARG and "chunks" in str(ei.value)


# ---- 11. the commitment ------------------------------------------------------------------------------------------------
def test_the_commitment_is_deterministic_and_depends_on_every_cell(p25):
    prep = cases.columns(3, 5)
    want = p25.p3_preprocessed_commit(prep, 2, threads=1).tolist()
    assert p25.p3_preprocessed_commit(prep.copy(), 2, threads=4).tolist() == want
    seen = {tuple(want)}
    for r in range(prep.shape[0]):
        for c in range(prep.shape[1]):
            other = prep.copy()
            other[r, c] = (int(other[r, c]) + 1) % P
            seen.add(tuple(p25.p3_preprocessed_commit(other, 2, threads=1).tolist()))
    assert len(seen) == 1 + prep.size
    assert p25.p3_preprocessed_commit(prep, 1, threads=1).tolist() != want       # another LDE domain, another key


# ---- 12-14. the verifier circuit -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def machine_outer(p25, oracle):
    air, trace, pv, prep, log_n, log_blowup = cases.make(p25, cases.shape("machine3"), x0=11)
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    c = p25.Circuit.build_p3_verifier_air(cfg, air)
    return air, cfg, inp, pv, prep, c, oracle.load_circuit(c.to_blob())


def test_oracle_proves_and_verifies_the_outer_circuit(machine_outer):
    air, cfg, inp, pv, prep, c, oc = machine_outer
    assert int(c.info.num_inputs) == inp.size
    wires, st, msg = oc.witness(inp, seed=3)
    assert st == 0, msg
    bad, msg = oc.check_constraints(wires)
    assert bad == 0, msg
    proof, st, _tm, msg = oc.prove(inp, seed=3)
    assert st == 0, msg
    assert proof[-2:].tolist() == [int(v) for v in pv]                        # the outer public inputs ARE the inner public values
    assert oc.verify(proof)[0] == 0


@pytest.mark.parametrize("cell", [(0, 0), (5, 1), (7, 0)])
def test_a_proof_under_other_columns_is_a_witness_conflict(p25, oracle, machine_outer, cell):
    """The circuit holds the commitment as constants: a valid proof made under columns that differ in one cell is observed
    under another key and its third batch opens into another tree."""
    air, cfg, inp, pv, prep, c, oc = machine_outer
    other = prep.copy()
    other[cell] = int(other[cell]) ^ 1 if cell[1] == 0 else (int(other[cell]) + 1) % P
    air2, trace2, pv2, _prep, _k, log_blowup = cases.make(p25, cases.shape("machine3"), x0=11, prep=other)
    inp2, cfg2 = _prove(p25, air2, trace2, pv2, log_blowup)
    assert bytes(cfg2) == bytes(cfg)
    assert oc.witness(inp2, seed=3)[1] == WITNESS_CONFLICT
    other_circuit = p25.Circuit.build_p3_verifier_air(cfg, air2)
    assert other_circuit.to_blob() != c.to_blob()
    oc2 = oracle.load_circuit(other_circuit.to_blob())
    assert oc2.witness(inp2, seed=3)[1] == 0 and oc2.witness(inp, seed=3)[1] == WITNESS_CONFLICT


def test_a_flipped_word_of_every_new_region_is_a_witness_conflict(p25, machine_outer):
    air, cfg, inp, pv, prep, c, oc = machine_outer
    for name, ranges in M.regions(cfg, prep.shape[1]).items():
        for lo, hi in (ranges[0], ranges[-1]):
            for o in sorted({lo, hi - 1}):
                bad = inp.copy()
                bad[o] = (int(bad[o]) + 1) % P
                assert oc.witness(bad, seed=3)[1] == WITNESS_CONFLICT, (name, o)
