"""GPU: checking a trace against its AIR on the device (include/p25.h "CHECKING A TRACE"): p25_p3_check_batch[_dev].

Every case of tests/air_cases_check.py: device report == host one-shot report == the independent model's
(tests/p3_check_model.py), word for word, and what the case's construction says of it.  Field arithmetic is exact: every
comparison is equality.

1. whens (public values, all four `when` kinds) at heights below a wave, one block, two blocks, 2^12: the variants of one
   height in one batch
2. auxiliary columns at one height below a wave, the scan block, twice it: AW 1 and 3, unbalanced multisets, zero denominators
3. periodic / preprocessed columns without auxiliary ones: the value tables made by the first check, and what they cost
4. the verdict is OK exactly when the prover proves the trace
5. five proofs in groups of two equal the lone calls; the device-resident form on guard-banded, stride-padded buffers;
   check_dev then prove_dev on one stream"""
import numpy as np
import pytest

import air_cases_check as cases
import p3_check_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK = 0
ODD = 4097
QUERIES, POW_BITS = 2, 4


def _groups(names):
    out = {}
    for name in names:
        out.setdefault(name.rsplit("_", 1)[0], []).append(name)
    return out


GROUPS = _groups(cases.NAMES)


def _prover(gpu, case):
    return gpu.P3Prover(case.air, case.log_n, case.log_blowup, QUERIES, POW_BITS)


def _pvs(group):
    return None if group[0].pv is None else np.stack([c.pv for c in group])


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2, 3 (reports), 4
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(GROUPS))
def test_device_report_is_the_hosts_and_the_models(gpu, oracle, key):
    """The variants of one AIR and height as one batch.  The last assertion -- verdict OK exactly when the device prover,
    from pow_start 0, returns P25_OK -- is a statement about these fixed traces, not a theorem: the prover's self-check is
    the quotient identity at one random point, which a violating trace passes with the STARK's soundness error."""
    group = [cases.build(gpu, name) for name in GROUPS[key]]
    pr = _prover(gpu, group[0])
    traces = np.stack([c.trace for c in group])
    reports = pr.check(traces, public_values=_pvs(group))
    for name, case, rep in zip(GROUPS[key], group, reports):
        host = gpu.p3_check_air(case.air, case.trace, case.pv, case.log_blowup, threads=1)
        model = M.report(oracle, gpu, case.air, case.trace, case.pv, case.log_blowup)
        assert rep.words == host.words == model, name
        cases.check_expectations(case, rep.words)
    _words, st = pr.prove(traces, public_values=_pvs(group), pow_starts=np.zeros(len(group), dtype=np.uint64))
    assert [s == OK for s in st.tolist()] == [rep.verdict == M.OK for rep in reports], GROUPS[key]
    if key.startswith("whens"):
        assert st.tolist()[GROUPS[key].index(key + "_d")] == OK          # an unread cell: the trace proves
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the value tables of a handle without auxiliary columns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["periodic", "preprocessed"])
def test_value_tables_are_made_by_the_first_check_only(gpu, kind):
    ok, flip = cases.build(gpu, kind + "_ok"), cases.build(gpu, kind + "_flip")
    pr, twin = _prover(gpu, ok), _prover(gpu, ok)
    assert pr.scratch_bytes() == twin.scratch_bytes() == (0, 0)
    want, st = twin.prove(ok.trace, public_values=ok.pv)
    got, st2 = pr.prove(ok.trace, public_values=ok.pv)
    assert st.tolist() == st2.tolist() == [OK] and np.array_equal(got, want)
    before = pr.scratch_bytes()
    assert before == twin.scratch_bytes()                                 # a handle that never checks holds what it held
    reps = pr.check(np.stack([ok.trace, flip.trace]), public_values=None if ok.pv is None else np.stack([ok.pv, flip.pv]))
    assert [r.verdict for r in reps] == [M.OK, M.VIOLATED]
    n = 1 << ok.log_n
    pw = 0 if ok.air.preprocessed is None else int(ok.air.preprocessed.shape[1])
    tables = 8 * (sum(len(c) for c in ok.air.periodic_columns) + pw * n)
    assert tables > 0
    after = pr.scratch_bytes()
    assert after[1] == before[1] and after[0] >= before[0] + tables       # the group of two may have grown the scratch too
    lone = pr.check(ok.trace, public_values=ok.pv)
    assert lone[0].words == reps[0].words and pr.scratch_bytes() == after  # made once
    got, st = pr.prove(ok.trace, public_values=ok.pv)                      # and the proving side is what it was
    assert st.tolist() == [OK] and np.array_equal(got, want)
    fresh = _prover(gpu, ok)                                               # a check as the handle's first call
    assert fresh.check(flip.trace, public_values=flip.pv)[0].words == reps[1].words
    got, st = fresh.prove(ok.trace, public_values=ok.pv)
    assert st.tolist() == [OK] and np.array_equal(got, want)
    for h in (pr, twin, fresh):
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. batches and the device-resident form
# ---------------------------------------------------------------------------------------------------------------------
FIVE_LOG_N = cases.AUX_HEIGHTS[2]


@pytest.fixture(scope="module")
def five(gpu, oracle):
    """Five traces of the det AIR at twice the scan block: satisfied, unbalanced, a zero denominator in the second block,
    satisfied (another seed), a zero denominator on row 0.  -> (air, traces[5], the model's reports[5])."""
    import air_cases_aux as aux
    air = aux.det_air(gpu)
    t = [aux.det_trace(FIVE_LOG_N, 0).copy() for _ in range(3)] + [aux.det_trace(FIVE_LOG_N, 1).copy() for _ in range(2)]
    t[1][5, 0] = (int(t[1][5, 0]) + 1) % P
    t[2][aux.SCAN_BLOCK + 3, 1] = 0
    t[4][0, 1] = 0
    want = [M.report(oracle, gpu, air, x, None, 1) for x in t]
    assert [w[0] for w in want] == [M.OK, M.VIOLATED, M.ZERO_DENOMINATOR, M.OK, M.ZERO_DENOMINATOR]
    traces = np.stack(t)
    traces.setflags(write=False)
    return air, traces, want


def _prover5(gpu, air):
    return gpu.P3Prover(air, FIVE_LOG_N, 1, QUERIES, POW_BITS)


def _two_proof_budget(pr, five):
    _air, traces, want = five
    assert pr.check(traces[:1])[0].words == want[0]
    per_proof = pr.scratch_bytes()[0]
    assert per_proof > 0
    return 2 * per_proof + per_proof // 2


def test_five_proofs_in_groups_of_two_equal_the_lone_calls(gpu, five):
    air, traces, want = five
    pr = _prover5(gpu, air)
    lone = [pr.check(traces[i:i + 1])[0].words for i in range(5)]
    assert lone == want
    assert [r.words for r in pr.check(traces)] == want                    # one group
    pr.close()
    pr = _prover5(gpu, air)
    budget = _two_proof_budget(pr, five)
    pr.set_scratch_budget(budget)
    assert [r.words for r in pr.check(traces)] == want                    # groups (0, 1), (2, 3), (4)
    assert budget * 2 // 5 < pr.scratch_bytes()[0] <= budget              # two proofs' worth, not one, not five
    order = np.array([4, 0, 3, 1, 2])
    assert [r.words for r in pr.check(traces[order])] == [want[i] for i in order]
    stride = pr.check_words + 3                                           # the host form leaves the words behind a report
    t = np.ascontiguousarray(traces)
    out = np.full((5, stride), 7, dtype=np.uint64)
    assert gpu.lib().p25_p3_check_batch(pr._h, t.ctypes.data, None, 5, out.ctypes.data, stride) == OK
    assert out[:, :pr.check_words].tolist() == want and (out[:, pr.check_words:] == 7).all()
    pr.close()


@pytest.mark.parametrize("grouped", [False, True])
def test_device_resident_batch_writes_check_words_per_proof(gpu, five, grouped):
    import torch
    air, traces, want = five
    pr = _prover5(gpu, air)
    if grouped:
        pr.set_scratch_budget(_two_proof_budget(pr, five))
    n, tw, cw = traces.shape[0], traces[0].size, pr.check_words
    r_stride, t_stride = cw + 5, tw + 3
    d_tr, d_rep = Banded(n * t_stride, before=ODD), Banded(n * r_stride, before=ODD)
    t_data, _t_pad = strided_rows(n, tw, t_stride)
    interior = d_tr.get()
    interior[t_data] = np.array(traces).reshape(-1)
    d_tr.set(interior)
    torch.cuda.synchronize()
    pr.check_dev(d_tr.ptr, t_stride, n, d_rep.ptr, r_stride)
    pr.sync()
    d_tr.assert_unchanged()
    d_rep.assert_bands_intact()
    r_data, r_pad = strided_rows(n, cw, r_stride)
    d_rep.assert_untouched(r_pad)
    assert d_rep.get()[r_data].reshape(n, cw).tolist() == want
    pr.close()


def test_check_then_prove_on_one_stream(gpu):
    """check_dev followed by prove_dev on one stream, no host synchronisation between them: both use the handle's one
    scratch, and both results are the separate calls'.  The whens AIR with public values, 2^9 rows, three traces."""
    import torch
    names = ["whens9_ok", "whens9_c", "whens9_d"]
    group = [cases.build(gpu, name) for name in names]
    traces, pvs = np.stack([c.trace for c in group]), _pvs(group)
    ref = _prover(gpu, group[0])
    want_rep = [r.words for r in ref.check(traces, public_values=pvs)]
    starts = np.zeros(3, dtype=np.uint64)
    want_words, want_st = ref.prove(traces, public_values=pvs, pow_starts=starts)
    assert want_st.tolist()[0] == want_st.tolist()[2] == OK != want_st.tolist()[1]
    ref.close()
    pr = _prover(gpu, group[0])
    n, tw, cw, ni, npub = 3, traces[0].size, pr.check_words, pr.num_inputs, 2
    d_tr, d_pv, d_ps = Banded(n * tw, before=ODD), Banded(n * npub, before=ODD), Banded(n, before=ODD)
    d_rep, d_in, d_st = Banded(n * cw, before=ODD), Banded(n * ni, before=ODD), Banded32(n, before=ODD)
    d_tr.set(traces.reshape(-1))
    d_pv.set(pvs.reshape(-1))
    d_ps.set(starts)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    pr.check_dev(d_tr.ptr, tw, n, d_rep.ptr, cw, stream=s.cuda_stream, d_public_values=d_pv.ptr)
    pr.prove_dev(d_tr.ptr, tw, n, d_ps.ptr, d_in.ptr, ni, d_st.ptr, stream=s.cuda_stream, d_public_values=d_pv.ptr)
    pr.check_dev(d_tr.ptr, tw, n, d_rep.ptr, cw, stream=s.cuda_stream, d_public_values=d_pv.ptr)   # and behind it again
    s.synchronize()
    for b in (d_tr, d_pv, d_ps):
        b.assert_unchanged()
    for b in (d_rep, d_in, d_st):
        b.assert_bands_intact()
    assert d_rep.get().reshape(n, cw).tolist() == want_rep
    assert d_st.get().tolist() == want_st.tolist()
    assert np.array_equal(d_in.get().reshape(n, ni), want_words)
    pr.close()
