"""CPU: challenges and auxiliary running-sum columns of the inner STARK (include/p25.h, "AUXILIARY COLUMNS") -- the AIR form,
the host prover, the verifier-circuit builder.

After the trace is committed the prover samples challenges, builds running sums of num / den in F_p^2 from them, commits
those as a fourth matrix and only then samples alpha.  Expected verdicts come from the independent model
tests/p3_aux_model.py; the committed columns are compared with the model's statement of their definition; the outer circuit
is judged by the oracle, loaded from the exported blob.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import air_cases_aux as cases
import p3_aux_model as M
import p3_preprocessed_model as PM
from conftest import P

OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4


class AuxColumn(C.Structure):
    """p25_air_aux_column, stated from the header."""
    _fields_ = [("num", C.c_uint32), ("den", C.c_uint32)]


class Aux(C.Structure):
    """p25_air_aux, stated from the header."""
    _fields_ = [("n_challenges", C.c_uint32), ("width", C.c_uint32), ("columns", C.POINTER(AuxColumn))]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _last(p25):
    return p25.lib().p25_last_error().decode()


def _prove(p25, air, trace, pv, log_blowup, queries=3, pow_bits=4, threads=1):
    return p25.p3_prove_air(air, trace, num_queries=queries, pow_bits=pow_bits, log_blowup=log_blowup, threads=threads,
                            public_values=pv)


def _key(p25, air, log_blowup):
    return None if air.preprocessed is None else p25.p3_preprocessed_commit(air.preprocessed, log_blowup, threads=1)


def _pw(air):
    return 0 if air.preprocessed is None else int(air.preprocessed.shape[1])


# ---- the host prover against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_host_prover_words_pass_the_model(p25, oracle, shape):
    air, trace, pv, log_n, log_blowup = cases.make(p25, shape)
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    assert cfg.log_trace_height == log_n
    aw = len(air.aux_columns)
    assert inp.size == M.num_inputs_formula(cfg, _pw(air), aw, air.n_public) == M.Shape(cfg, _pw(air), aw).num_inputs + air.n_public
    assert M.verify(oracle, air, cfg, inp, _key(p25, air, log_blowup)) == M.OK
    assert int(p25.Circuit.build_p3_verifier_air(cfg, air).info.num_inputs) == inp.size


@pytest.mark.parametrize("name", ["perm", "range", "tuple", "wide", "det", "pvper", "perm_b2"])
def test_the_committed_columns_are_the_running_sums(p25, oracle, name):
    """aux_commit against the definition: the challenges from the model's transcript, the running sums term by term in
    Python integers, split into components, committed as the model commits a matrix."""
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape(name))
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    aw = len(air.aux_columns)
    s = M.Shape(cfg, _pw(air), aw)
    chal = M.challenges_of(oracle, air, inp, cfg, _key(p25, air, log_blowup))
    sums = M.running_sums(air, trace, [int(v) for v in pv] if pv is not None else [], chal)
    assert sums[0] == [(0, 0)] * aw
    matrix = np.array([[c for v in row for c in v] for row in sums], dtype=np.uint64)
    assert matrix.shape == (1 << log_n, 2 * aw)
    assert inp[s.o_aux_commit:s.o_aux_commit + 4].tolist() == PM.model_commit(oracle, matrix, log_blowup)


def test_big_heights_pass_the_model(p25, oracle):
    """The heights on either side of the device scan's second totals tile: 2 queries, no proof of work, 16 threads."""
    for shp in cases.BIG_SHAPES:
        air, trace, pv, log_n, log_blowup = cases.make(p25, shp)
        inp, cfg = _prove(p25, air, trace, pv, log_blowup, queries=2, pow_bits=0, threads=16)
        assert M.verify(oracle, air, cfg, inp) == M.OK


# ---- single-word flips in every new region: the model's verdict, and the oracle's copy of the circuit ---------------------
@pytest.fixture(scope="module", params=["range", "wide", "pvper"])
def outer(request, p25, oracle):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape(request.param))
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    c = p25.Circuit.build_p3_verifier_air(cfg, air)
    return air, cfg, inp, _key(p25, air, log_blowup), oracle.load_circuit(c.to_blob())


def test_oracle_witnesses_the_outer_circuit(outer):
    air, cfg, inp, key, oc = outer
    wires, st, msg = oc.witness(inp, seed=3)
    assert st == 0, msg
    bad, msg = oc.check_constraints(wires)
    assert bad == 0, msg


def test_flips_in_every_new_region(oracle, outer):
    air, cfg, inp, key, oc = outer
    flips = []
    for name, ranges in M.regions(cfg, _pw(air), len(air.aux_columns)).items():
        spans = ranges if name in ("row", "path") else ranges[:1]
        for lo, hi in spans:
            flips += [(name, o) for o in sorted({lo, hi - 1})]
    for name, o in flips:
        bad = inp.copy()
        bad[o] = (int(bad[o]) + 1) % P
        verdict = M.verify(oracle, air, cfg, bad, key)
        assert verdict != M.OK, (name, o)
        if name in ("row", "path"):
            assert verdict == M.INPUT_MERKLE, (name, o)
        # the circuit has a witness exactly for OK
        assert oc.witness(bad, seed=3)[1] == WITNESS_CONFLICT, (name, o)


def test_a_circuit_for_another_num_node_rejects(p25, oracle):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape("perm"))
    inp, cfg = _prove(p25, air, trace, pv, log_blowup)
    oc = oracle.load_circuit(p25.Circuit.build_p3_verifier_air(cfg, air).to_blob())
    assert oc.witness(inp, seed=3)[1] == 0
    # a verifier does not read num / den -- the constraints state them: an AIR whose constraint reads another numerator
    other = p25.Air(2, aux=1)
    a, b, g = other.local(0), other.local(1), other.challenge(0)
    num, den = a, other.mul(other.sub(g, a), other.sub(g, b))
    other.aux_column(num, den)
    cases._running_sum_constraints(other, 0, num, den)
    assert M.verify(oracle, other, cfg, inp) == M.CONSTRAINTS
    oc2 = oracle.load_circuit(p25.Circuit.build_p3_verifier_air(cfg, other).to_blob())
    assert oc2.witness(inp, seed=3)[1] == WITNESS_CONFLICT


# ---- what the prover refuses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["perm", "wide", "perm_b2", "perm_block"])
def test_a_column_that_is_no_permutation_is_refused(p25, name):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape(name))
    with pytest.raises(p25.P25Error) as ei:
        _prove(p25, air, cases.not_a_permutation(trace), pv, log_blowup)
    assert ei.value.status == INVALID_ARG and "quotient identity" in str(ei.value)


@pytest.mark.parametrize("name", ["range", "tuple", "pvper"])
def test_a_wrong_multiplicity_is_refused(p25, name):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape(name))
    bad = trace.copy()
    bad[1, trace.shape[1] - 1] = (int(bad[1, trace.shape[1] - 1]) + 1) % P
    with pytest.raises(p25.P25Error) as ei:
        _prove(p25, air, bad, pv, log_blowup)
    assert ei.value.status == INVALID_ARG and "quotient identity" in str(ei.value)


@pytest.mark.parametrize("row", [0, 5, 7])
def test_a_zero_denominator_names_column_and_row(p25, row):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape("det"))
    bad = trace.copy()
    bad[row, 1] = 0
    with pytest.raises(p25.P25Error) as ei:
        _prove(p25, air, bad, pv, log_blowup)
    msg = str(ei.value)
    assert ei.value.status == INVALID_ARG and "zero denominator" in msg and "column 0" in msg and "row %d" % row in msg


# ---- aux = NULL: the _pp functions, byte for byte ------------------------------------------------------------------------
def test_no_aux_reproduces_the_pp_words_and_the_blob(p25):
    import air_cases_preprocessed as prep_cases
    lib = p25.lib()
    air, trace, pv, prep, log_n, log_blowup = prep_cases.make(p25, prep_cases.shape("machine2_per"))
    want, cfg = p25.p3_prove_air(air, trace, num_queries=4, pow_bits=5, log_blowup=log_blowup, threads=1, public_values=pv)
    want_blob = p25.Circuit.build_p3_verifier_air(cfg, air).to_blob()
    ac, pc, pp = air.to_c(), air.periodic_to_c(), air.preprocessed_to_c()
    dummy = (AuxColumn * 1)(AuxColumn(0, 0))
    for aux in (None, C.byref(Aux(0, 0, None)), C.byref(Aux(0, 0, dummy))):
        n, c2 = C.c_size_t(0), p25.P3Config()
        assert lib.p25_p3_prove_air_ax(C.byref(ac), _p(trace), _p(pv), C.byref(pc), C.byref(pp), aux, log_n, log_blowup, 4, 5, 0, 1,
                                       None, 0, C.byref(n), C.byref(c2)) == OK, _last(p25)
        assert n.value == want.size
        out = np.zeros(n.value, dtype=np.uint64)
        assert lib.p25_p3_prove_air_ax(C.byref(ac), _p(trace), _p(pv), C.byref(pc), C.byref(pp), aux, log_n, log_blowup, 4, 5, 0, 1,
                                       _p(out), out.size, C.byref(n), C.byref(c2)) == OK, _last(p25)
        assert (out == want).all() and bytes(c2) == bytes(cfg)
        h = C.c_void_p()
        assert lib.p25_circuit_build_p3_verifier_air_ax(C.byref(cfg), C.byref(ac), C.byref(pc), C.byref(pp), aux, C.byref(h)) == OK
        assert p25.Circuit(h.value).to_blob() == want_blob
        h = C.c_void_p()
        assert lib.p25_p3_prover_create_ax(C.byref(ac), C.byref(pc), C.byref(pp), aux, log_n, log_blowup, 4, 5, C.byref(h)) == OK
        c3, n3 = p25.P3Config(), C.c_size_t(0)
        assert lib.p25_p3_prover_config(h, C.byref(c3), C.byref(n3)) == OK
        lib.p25_p3_prover_destroy(h)
        assert bytes(c3) == bytes(cfg) and n3.value == want.size


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _entry_points(p25, air, n_challenges, columns, log_n=3):
    """The three _ax entry points on `air` with a raw p25_air_aux -> [(status, message)]; nothing may be written."""
    lib = p25.lib()
    ac = air.to_c()
    cols = (AuxColumn * max(1, len(columns)))(*[AuxColumn(n, d) for n, d in columns])
    aux = Aux(n_challenges, len(columns), cols)
    trace = np.ones((1 << log_n, air.width), dtype=np.uint64)
    out = np.zeros(1 << 14, dtype=np.uint64)
    res = []
    n = C.c_size_t(12345)
    st = lib.p25_p3_prove_air_ax(C.byref(ac), _p(trace), None, None, None, C.byref(aux), log_n, 1, 3, 4, 0, 1, _p(out), out.size,
                                 C.byref(n), None)
    res.append((st, _last(p25)))
    assert n.value == 12345 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create_ax(C.byref(ac), None, None, C.byref(aux), log_n, 1, 3, 4, C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    cfg = p25.P3Config(1, 3, 4, 0, log_n, air.width, log_n + 1, 2, log_n)
    st = lib.p25_circuit_build_p3_verifier_air_ax(C.byref(cfg), C.byref(ac), None, None, C.byref(aux), C.byref(h))
    res.append((st, _last(p25)))
    assert not h.value
    return res


def _plain(p25, extra=None):
    """local0 - local1 = 0, and the nodes `extra` adds -> (air, what extra returned)."""
    air = p25.Air(2)
    got = extra(air) if extra else None
    air.assert_zero(air.sub(air.local(0), air.local(1)))
    return air, got


@pytest.mark.parametrize("name,build,n_challenges,columns,word", [
    ("num depends on AUX_LOCAL", lambda a: a.add(a.aux_local(0), a.local(0)), 0, lambda x: [(x, 1)], "AUX_LOCAL"),
    ("den depends on AUX_NEXT", lambda a: a.mul(a.local(0), a.aux_next(0)), 0, lambda x: [(0, x)], "AUX_NEXT"),
    ("CHALLENGE index = n_challenges", lambda a: a.challenge(1), 1, lambda x: [(0, 1)], "n_challenges"),
    ("AUX_LOCAL index = width", lambda a: a.aux_local(1), 0, lambda x: [(0, 1)], "width"),
    ("AUX_NEXT index = width", lambda a: a.aux_next(2), 0, lambda x: [(0, 1), (0, 1)], "width"),
    ("num node out of range", None, 0, lambda x: [(1000, 0)], "n_nodes"),
    ("den node out of range", None, 0, lambda x: [(0, 1000)], "n_nodes"),
    ("challenges without columns", None, 2, lambda x: [], "width = 0"),
    ("9 challenges", None, 9, lambda x: [(0, 1)], "P25_AIR_MAX_CHALLENGES"),
    ("17 columns", None, 0, lambda x: [(0, 1)] * 17, "P25_AIR_MAX_AUX"),
])
def test_refusals_name_the_limit(p25, name, build, n_challenges, columns, word):
    def extra(air):
        air.local(0), air.local(1)           # nodes 0 and 1: what the plain column descriptions refer to
        return build(air) if build else None
    air, got = _plain(p25, extra)
    for st, msg in _entry_points(p25, air, n_challenges, columns(got)):
        assert st == INVALID_ARG and word in msg, (name, st, msg)


def test_the_caps_themselves_are_accepted(p25, oracle):
    """8 challenges and 16 columns; and columns without a challenge (det) prove."""
    air = p25.Air(2, aux=8)
    a, b = air.local(0), air.local(1)
    g = air.challenge(0)
    for i in range(1, 8):
        g = air.add(g, air.challenge(i))
    for j in range(16):
        gj = air.add(g, air.const(j))
        num, den = air.sub(a, b), air.mul(air.sub(gj, a), air.sub(gj, b))
        air.aux_column(num, den)
        cases._running_sum_constraints(air, j, num, den)
    inp, cfg = _prove(p25, air, cases.perm_trace(3), None, 1)
    assert inp.size == M.num_inputs_formula(cfg, 0, 16, 0)
    assert M.verify(oracle, air, cfg, inp) == M.OK


@pytest.mark.parametrize("op", [10, 11, 12])
def test_the_forms_without_aux_refuse_the_ops_and_write_nothing(p25, op):
    lib = p25.lib()
    air = p25.Air(2)
    x = {10: air.challenge, 11: air.aux_local, 12: air.aux_next}[op](0)
    air.assert_zero(air.sub(air.local(1), air.mul(air.local(0), x)))
    ac = air.to_c()
    trace = np.zeros((8, 2), dtype=np.uint64)
    out = np.zeros(4096, dtype=np.uint64)
    n = C.c_size_t(777)
    args = (3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    st = lib.p25_p3_prove_air(C.byref(ac), _p(trace), 3, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_ax" in _last(p25)
    st = lib.p25_p3_prove_air_ex(C.byref(ac), _p(trace), *args)
    assert st == INVALID_ARG and "p25_p3_prove_air_ax" in _last(p25)
    st = lib.p25_p3_prove_air_pv(C.byref(ac), _p(trace), None, *args)
    assert st == INVALID_ARG and "p25_p3_prove_air_ax" in _last(p25)
    st = lib.p25_p3_prove_air_pc(C.byref(ac), _p(trace), None, None, *args)
    assert st == INVALID_ARG and "p25_p3_prove_air_ax" in _last(p25)
    st = lib.p25_p3_prove_air_pp(C.byref(ac), _p(trace), None, None, None, *args)
    assert st == INVALID_ARG and "p25_p3_prove_air_ax" in _last(p25)
    assert n.value == 777 and not out.any()
    h = C.c_void_p(0)
    st = lib.p25_p3_prover_create(C.byref(ac), 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_ax" in _last(p25) and not h.value
    st = lib.p25_p3_prover_create_pc(C.byref(ac), None, 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_ax" in _last(p25) and not h.value
    st = lib.p25_p3_prover_create_pp(C.byref(ac), None, None, 3, 1, 3, 4, C.byref(h))
    assert st == INVALID_ARG and "p25_p3_prover_create_ax" in _last(p25) and not h.value
    cfg = p25.P3Config(1, 3, 4, 0, 3, 2, 4, 2, 3)
    st = lib.p25_circuit_build_p3_verifier_air(C.byref(cfg), C.byref(ac), C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_ax" in _last(p25) and not h.value
    st = lib.p25_circuit_build_p3_verifier_air_pc(C.byref(cfg), C.byref(ac), None, C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_ax" in _last(p25) and not h.value
    st = lib.p25_circuit_build_p3_verifier_air_pp(C.byref(cfg), C.byref(ac), None, None, C.byref(h))
    assert st == INVALID_ARG and "p25_circuit_build_p3_verifier_air_ax" in _last(p25) and not h.value


# ---- degree ------------------------------------------------------------------------------------------------------------
def test_aux_ops_count_as_degree_one_and_challenges_as_zero(p25):
    lib = p25.lib()
    for build, lqd in ((lambda a, x: a.mul(a.aux_local(0), a.mul(x, x)), 1),                   # AUX * LOCAL * LOCAL: 3
                       (lambda a, x: a.mul(a.aux_next(0), x), 0),                              # degree 2: one chunk
                       (lambda a, x: a.mul(a.challenge(0), a.mul(a.aux_next(0), x)), 0)):      # a challenge adds nothing
        air = p25.Air(2, aux=1)
        x = air.local(0)
        air.aux_column(x, air.local(1))
        air.assert_zero(air.sub(build(air, x), air.local(1)))
        ac, ax = air.to_c(), air.aux_to_c()
        n, cfg = C.c_size_t(0), p25.P3Config()
        assert lib.p25_p3_prove_air_ax(C.byref(ac), None, None, None, None, C.byref(ax), 3, 2, 3, 4, 0, 1, None, 0, C.byref(n),
                                       C.byref(cfg)) == OK, _last(p25)
        assert cfg.log_quotient_degree == lqd


# ---- the device verifier's lane functions, on the host ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes(p25, tmp_path_factory):
    """tests/native/p3_verify_lanes_aux.cpp: the lanes of plonky2.5_amd/csrc/p3_verify_lanes.h in plain loops, under
    AddressSanitizer and UBSan (host code, a stand-alone program)."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    p25.lib()
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp("p3_verify_lanes_aux")
    exe = str(d / "p3_verify_lanes_aux")
    libdir = os.path.dirname(p25.binding.lib_path)
    csrc = os.path.join(ROOT, "plonky2.5_amd", "csrc")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "p3_verify_lanes_aux.cpp"),
                        "-o", exe, "-L" + libdir, "-lp25", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(air, log_n, log_blowup, queries, pow_bits, proofs):
        data = str(d / "batch.bin")
        head = [air.width, len(air.nodes), len(air.constraints), log_n, log_blowup, queries, pow_bits, len(proofs),
                air.n_challenges, len(air.aux_columns)]
        with open(data, "wb") as f:
            for part in (head, [x for nd in air.nodes for x in nd], [x for c in air.constraints for x in c],
                         [x for c in air.aux_columns for x in c], np.stack(proofs)):
                f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]
    return run


def flipped(inp, cfg, pw, aw, stride=11):
    """The proof, a flip of every stride-th word and of the first and last word of every new region."""
    at = set(range(0, inp.size, stride))
    for ranges in M.regions(cfg, pw, aw).values():
        for lo, hi in ranges:
            at |= {lo, hi - 1}
    out = [inp]
    for o in sorted(at):
        bad = inp.copy()
        bad[o] = (int(bad[o]) + 1) % P
        out.append(bad)
    return out


@pytest.mark.parametrize("name", ["perm", "tuple", "wide", "det", "perm_b2"])
def test_lanes_equal_the_model(p25, oracle, lanes, name):
    air, trace, pv, log_n, log_blowup = cases.make(p25, cases.shape(name))
    inp, cfg = _prove(p25, air, trace, pv, log_blowup, queries=2, pow_bits=3)
    proofs = flipped(inp, cfg, 0, len(air.aux_columns))
    proofs += [np.full(inp.size, (1 << 64) - 1, dtype=np.uint64), np.zeros_like(inp)]
    want = [M.verify(oracle, air, cfg, w) for w in proofs]
    assert want[0] == M.OK and M.OK not in want[1:]
    assert {M.MALFORMED, M.INPUT_MERKLE, M.FRI_MERKLE} <= set(want)   # an opening's flip shows at the first FRI leaf
    assert lanes(air, log_n, log_blowup, 2, 3, proofs) == want


def test_the_stage_timer_refuses_a_handle_that_has_not_proved(p25):
    for name in ("perm", None):
        air = cases.make(p25, cases.shape(name))[0] if name else p25.Air.fibonacci()
        pr = p25.P3Prover(air, 3, 1, 3, 4)
        with pytest.raises(p25.P25Error) as ei:
            pr.aux_stage_ms()
        assert ei.value.status == INVALID_ARG and "p25_p3_prover_aux_stage_ms" in str(ei.value)
        pr.close()
