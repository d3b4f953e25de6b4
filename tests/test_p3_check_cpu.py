"""CPU: checking a trace against its AIR (include/p25.h "CHECKING A TRACE") -- the host one-shot p25_p3_check_air_ax, the
argument errors of the batch entry points, and the lane functions as a stand-alone program under the sanitizers.

Expected reports come from the independent model tests/p3_check_model.py, word for word; what each case's construction says
of its report is asserted beside that (tests/air_cases_check.py).  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import air_cases_check as cases
import p3_check_model as M
from conftest import P

OK, INVALID_ARG, NO_DEVICE = 0, 1, 2


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def want(p25, oracle):
    """The model's report of a case, computed once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            case = cases.build(p25, name)
            memo[name] = (case, M.report(oracle, p25, case.air, case.trace, case.pv, case.log_blowup))
        return memo[name]
    return get


# ---- the host one-shot against the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_host_report_is_the_models(p25, want, name):
    case, model = want(name)
    rep = p25.p3_check_air(case.air, case.trace, case.pv, case.log_blowup, threads=1)
    assert rep.words == model
    cases.check_expectations(case, rep.words)
    aw = len(case.air.aux_columns)
    assert rep.verdict == model[0] and rep.n_violations == model[1] and rep.counts == model[8 + 2 * aw:]
    assert rep.first == (None if model[2] == M.NONE else (model[2], model[3]))
    assert rep.zero_denominator == (None if model[4] == M.NONE else (model[4], model[5]))
    assert [x for t in rep.totals for x in t] == model[8:8 + 2 * aw]


def test_the_report_does_not_depend_on_the_threads(p25):
    case = cases.build(p25, "perm3_9_notperm")
    one = p25.p3_check_air(case.air, case.trace, case.pv, case.log_blowup, threads=1)
    many = p25.p3_check_air(case.air, case.trace, case.pv, case.log_blowup, threads=7)
    assert one.words == many.words


def test_the_challenges_hang_on_log_blowup(p25, oracle):
    """The totals of an unbalanced column are a function of the challenge, which the trace's commitment decides."""
    case = cases.build(p25, "perm1_5_notperm")
    reps = [p25.p3_check_air(case.air, case.trace, None, B, threads=1) for B in (2, 3)]
    assert reps[0].totals != reps[1].totals and reps[0].counts == reps[1].counts
    for B, rep in zip((2, 3), reps):
        assert rep.words == M.report(oracle, p25, case.air, case.trace, None, B)


# ---- the one-shot's arguments -------------------------------------------------------------------------------------------
def _one_shot(p25, case, trace=True, pv=True, report=True, cap=None, words=True, air=True, log_n=None):
    ac, pc, pp, ax = case.air.to_c(), case.air.periodic_to_c(), case.air.preprocessed_to_c(), case.air.aux_to_c()
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    t = np.ascontiguousarray(case.trace, dtype=np.uint64)
    v = None if case.pv is None else np.ascontiguousarray(case.pv, dtype=np.uint64)
    n = C.c_size_t(0)
    need = 8 + 2 * len(case.air.aux_columns) + len(case.air.constraints)
    out = np.zeros(need if cap is None else max(cap, 1), dtype=np.uint64)
    st = p25.lib().p25_p3_check_air_ax(C.byref(ac) if air else None, ref(pc), ref(pp), ref(ax), _p(t) if trace else None,
                                       _p(v) if pv else None, case.log_n if log_n is None else log_n, case.log_blowup, 1,
                                       _p(out) if report else None, need if cap is None else cap,
                                       C.byref(n) if words else None)
    return st, int(n.value), out


def test_one_shot_argument_errors(p25):
    case = cases.build(p25, "whens3_a0")
    need = 8 + len(case.air.constraints)
    assert _one_shot(p25, case)[:2] == (OK, need)
    st, n, out = _one_shot(p25, case, report=False)                   # the size query needs no trace
    assert (st, n) == (OK, need) and not out.any()
    assert _one_shot(p25, case, report=False, trace=False)[:2] == (OK, need)
    assert _one_shot(p25, case, air=False)[0] == INVALID_ARG
    assert _one_shot(p25, case, words=False)[0] == INVALID_ARG
    assert _one_shot(p25, case, trace=False)[0] == INVALID_ARG
    assert _one_shot(p25, case, pv=False)[0] == INVALID_ARG           # n_public = 2 and no public values
    assert _one_shot(p25, case, cap=need - 1)[0] == INVALID_ARG
    assert _one_shot(p25, case, log_n=0)[0] == INVALID_ARG
    bad = case._replace(trace=case.trace.copy())
    bad.trace[1, 0] = P
    assert _one_shot(p25, bad)[0] == INVALID_ARG
    bad = case._replace(pv=np.array([int(case.pv[0]), P], dtype=np.uint64))
    assert _one_shot(p25, bad)[0] == INVALID_ARG
    nopub = cases.build(p25, "perm1_5_ok")                            # n_public = 0 and public values
    assert _one_shot(p25, nopub._replace(pv=np.zeros(2, dtype=np.uint64)))[0] == INVALID_ARG


# ---- the batch entry points' arguments: all refused, or answered, before any device is looked for ---------------------------
@pytest.fixture(scope="module")
def handle(p25):
    case = cases.build(p25, "whens3_ok")
    pr = p25.P3Prover(case.air, case.log_n, 1, num_queries=2, pow_bits=0)
    yield case, pr
    pr.close()


def test_check_words(p25, handle):
    case, pr = handle
    n = C.c_size_t(0)
    assert p25.lib().p25_p3_prover_check_words(pr._h, C.byref(n)) == OK and n.value == 8 + 4 == pr.check_words
    assert p25.lib().p25_p3_prover_check_words(None, C.byref(n)) == INVALID_ARG
    assert p25.lib().p25_p3_prover_check_words(pr._h, None) == INVALID_ARG
    ax = cases.build(p25, "perm3_5_ok")
    pa = p25.P3Prover(ax.air, ax.log_n, 1, num_queries=2, pow_bits=0)
    assert pa.check_words == 8 + 2 * 3 + 6
    pa.close()


def test_batch_argument_errors(p25, handle):
    case, pr = handle
    lib = p25.lib()
    t = np.ascontiguousarray(np.stack([case.trace, case.trace]), dtype=np.uint64)
    pv = np.ascontiguousarray(np.stack([case.pv, case.pv]), dtype=np.uint64)
    cw, tw = pr.check_words, t[0].size
    out = np.full(2 * cw, 7, dtype=np.uint64)
    host = lambda h=pr._h, tr=t, v=pv, n=2, o=out, s=cw: lib.p25_p3_check_batch(h, _p(tr), _p(v), n, _p(o), s)   # noqa: E731
    dev = lambda h=pr._h, tr=t, ts=tw, v=pv, n=2, o=out, s=cw: \
        lib.p25_p3_check_batch_dev(h, _p(tr), ts, _p(v), n, _p(o), s, None)   # noqa: E731
    for call in (host, dev):
        assert call(h=None) == INVALID_ARG
        assert call(n=0) == OK                                        # nothing touched, no device needed
        assert call(n=0, tr=None, v=None, o=None) == OK
        assert call(tr=None) == INVALID_ARG
        assert call(o=None) == INVALID_ARG
        assert call(v=None) == INVALID_ARG                            # the AIR has public values
        assert call(s=cw - 1) == INVALID_ARG
        assert call(n=(1 << 24) + 1) == INVALID_ARG
    assert dev(ts=tw - 1) == INVALID_ARG
    bad = t.copy()
    bad[1, 3, 1] = P                                                  # a word >= p fails the whole call before any launch
    assert host(tr=bad) == INVALID_ARG
    badv = pv.copy()
    badv[0, 1] = P + 5
    assert host(v=badv) == INVALID_ARG
    assert (out == 7).all()
    nopub = cases.build(p25, "perm1_5_ok")                            # public values for an AIR that has none
    pa = p25.P3Prover(nopub.air, nopub.log_n, 1, num_queries=2, pow_bits=0)
    tr = np.ascontiguousarray(nopub.trace.reshape((1,) + nopub.trace.shape))
    o = np.zeros(pa.check_words, dtype=np.uint64)
    assert lib.p25_p3_check_batch(pa._h, _p(tr), _p(pv), 1, _p(o), pa.check_words) == INVALID_ARG
    assert lib.p25_p3_check_batch_dev(pa._h, _p(tr), tr.size, _p(pv), 1, _p(o), pa.check_words, None) == INVALID_ARG
    pa.close()


def test_a_valid_call_needs_a_device(p25, handle):
    """Argument errors come first, then P25_ERR_NO_DEVICE: the batch forms have no CPU path (the one-shot is it).  Where a
    device is present there is nothing to assert here: tests/test_gpu_p3_check.py holds the answers of a valid call."""
    import torch
    if torch.cuda.is_available():
        return
    case, pr = handle
    with pytest.raises(p25.P25Error) as e:
        pr.check(case.trace, public_values=case.pv)
    assert e.value.status == NO_DEVICE
    assert pr.scratch_bytes() == (0, 0)


# ---- the lane functions in plain loops, under the sanitizers ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes(p25, tmp_path_factory):
    """tests/native/p3_check_lanes.cpp: the lanes of plonky2.5_amd/csrc/p3_check_lanes.h in plain loops, under
    AddressSanitizer and UBSan (host code, a stand-alone program)."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    p25.lib()
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp("p3_check_lanes")
    exe = str(d / "p3_check_lanes")
    libdir = os.path.dirname(p25.binding.lib_path)
    csrc = os.path.join(ROOT, "plonky2.5_amd", "csrc")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "p3_check_lanes.cpp"),
                        "-o", exe, "-L" + libdir, "-lp25", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(case, challenges):
        air = case.air
        data = str(d / "case.bin")
        pw = 0 if air.preprocessed is None else int(air.preprocessed.shape[1])
        head = [air.width, len(air.nodes), len(air.constraints), case.log_n, case.log_blowup, air.n_public, air.n_challenges,
                len(air.aux_columns), len(air.periodic_columns), pw]
        per = [x for c in air.periodic_columns for x in [len(c).bit_length() - 1] + [int(v) for v in c]]
        parts = [head, [x for nd in air.nodes for x in nd], [x for c in air.constraints for x in c],
                 [x for c in air.aux_columns for x in c], per,
                 [] if air.preprocessed is None else np.asarray(air.preprocessed, dtype=np.uint64).ravel(),
                 [] if case.pv is None else case.pv, [x for c in challenges for x in c], np.asarray(case.trace).ravel()]
        with open(data, "wb") as f:
            for part in parts:
                f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]
    return run


LANE_CASES = ["whens3_c", "whens6_a63", "whens9_e", "whens9_d", "perm1_5_notperm", "perm3_8_ok", "det_9_zero257", "det_5_ok",
              "range_8_ok", "tuple_5_ok", "pvper_9_ok", "periodic_flip", "preprocessed_flip"]


@pytest.mark.parametrize("name", LANE_CASES)
def test_lane_functions_give_the_models_report(p25, oracle, want, lanes, name):
    case, model = want(name)
    pv = [int(v) for v in case.pv] if case.pv is not None else []
    chal = M.challenges(oracle, p25, case.air, case.trace, pv, case.log_blowup)
    assert lanes(case, chal) == model
