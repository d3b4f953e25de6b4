"""GPU: public values of the inner STARK on the device (include/p25.h, "PUBLIC VALUES"): p25_p3_prove_batch_pv[_dev],
p25_p3_verify_batch[_dev] on proofs that end in their public values, the outer proof whose public inputs they become, and
an aggregate that commits to them.  Field arithmetic is exact: every comparison is equality.

1. the device prover's words are the host prover's, for each shape at which a path differs (the challenger's rate of 4
   filled and crossed by the values observed behind the 4-word trace root; 64 values; log_blowup 2; one row pair)
2. a batch in groups: every proof reads ITS row of public values, whichever group it runs in; a failed proof is zeros
3. the verifier's verdict equals the independent model's (tests/p3_public_values_model.py) for a mutation of every section
4. the outer proof equals the oracle's, ends in [a, b, x], and a changed public value is a witness conflict; the chain
   prove -> verify -> outer prove on one stream
5. a 2-to-1 aggregate's public inputs are hash_no_pad(pv0 || pv1)"""
import numpy as np
import pytest

import air_cases_pv
import p3_public_values_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097

# name -> (log_n, log_blowup, queries, pow_bits)
FIB_SHAPES = {"fib_1_1_0_1": (1, 1, 1, 0), "fib_3_4_8_1": (3, 1, 4, 8), "fib_6_4_8_2": (6, 2, 4, 8)}
MIX_M = (1, 3, 4, 5, 12, 13, 64)
CASE_KEYS = list(FIB_SHAPES) + ["mix_%d" % m for m in MIX_M]


class Case:
    """An AIR with public values, one satisfying (trace, public values) and the HOST prover's flat proof of them."""

    def __init__(self, p25, key):
        if key.startswith("fib"):
            self.log_n, self.log_blowup, self.queries, self.pow_bits = FIB_SHAPES[key]
            self.air = air_cases_pv.fib_pv(p25)
            self.trace, self.pv = air_cases_pv.fib_pv_trace(self.log_n, 11 + self.log_n, (1 << 63) + 5)
        else:
            m = int(key.split("_")[1])
            self.log_n, self.log_blowup, self.queries, self.pow_bits = 3, 1, 2, 3
            self.air = air_cases_pv.pv_mix(p25, m)
            self.pv = air_cases_pv.pv_mix_values(m, 1)
            self.trace = air_cases_pv.pv_mix_trace(3, self.pv)
        self.words, self.cfg = p25.p3_prove_air(self.air, self.trace, num_queries=self.queries, pow_bits=self.pow_bits,
                                                log_blowup=self.log_blowup, threads=1, public_values=self.pv)
        self.shape = M.Shape(self.cfg)
        self.m = self.air.n_public
        assert self.words.size == self.shape.num_inputs + self.m
        self.words.setflags(write=False)

    def prover(self, p25):
        return p25.P3Prover(self.air, self.log_n, self.log_blowup, self.queries, self.pow_bits)


_cases = {}


def case_of(p25, key):
    if key not in _cases:
        _cases[key] = Case(p25, key)
    return _cases[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. device == host, word for word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASE_KEYS)
def test_device_words_are_the_host_words(gpu, key):
    case = case_of(gpu, key)
    pr = case.prover(gpu)
    assert pr.n_public == case.m and pr.num_inputs == case.words.size
    got, st = pr.prove(case.trace, public_values=case.pv)
    assert st.tolist() == [OK]
    assert np.array_equal(got[0, -case.m:], case.pv)
    assert np.array_equal(got[0], case.words), np.nonzero(got[0] != case.words)[0][:8]
    # the forms without public values refuse this handle; nothing is written
    out = np.zeros((1, pr.num_inputs), dtype=np.uint64)
    st32 = np.full(1, 77, dtype=np.int32)
    tr = np.ascontiguousarray(case.trace)
    rc = gpu.lib().p25_p3_prove_batch(pr._h, tr.ctypes.data, 1, None, out.ctypes.data, pr.num_inputs, st32.ctypes.data)
    assert rc == INVALID_ARG and "p25_p3_prove_batch_pv" in gpu.lib().p25_last_error().decode()
    assert not out.any() and st32.tolist() == [77]
    pr.close()


def test_pv_forms_without_public_values_are_the_plain_forms(gpu):
    """n_public = 0: public_values NULL, the words of p25_p3_prove_batch."""
    import air_cases
    air, trace = gpu.Air.fibonacci(), air_cases.fib_trace(3)
    pr = gpu.P3Prover(air, 3, 1, 4, 8)
    want, st = pr.prove(trace)
    assert st.tolist() == [OK]
    out = np.zeros((1, pr.num_inputs), dtype=np.uint64)
    st32 = np.full(1, 77, dtype=np.int32)
    tr = np.ascontiguousarray(trace)
    rc = gpu.lib().p25_p3_prove_batch_pv(pr._h, tr.ctypes.data, None, 1, None, out.ctypes.data, pr.num_inputs, st32.ctypes.data)
    assert rc == OK and st32.tolist() == [OK] and np.array_equal(out, want)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. a batch with groups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fib5(gpu):
    """Five fib_pv instances (3, 4 queries, 8 PoW bits) with distinct public values; proof 2's trace disagrees with its
    pv2.  -> (air, traces[5], pvs[5][3], pow_starts, host rows[5] with row 2 zeros)."""
    air = air_cases_pv.fib_pv(gpu)
    traces, pvs, rows = [], [], []
    starts = np.array([0, 1 << 20, 5, 7 << 30, 3], dtype=np.uint64)
    for i in range(5):
        t, pv = air_cases_pv.fib_pv_trace(3, 100 + 7 * i, 3 + i)
        if i == 2:
            pv[2] = (int(pv[2]) + 1) % P
            with pytest.raises(gpu.P25Error) as e:
                gpu.p3_prove_air(air, t, num_queries=4, pow_bits=8, pow_start=int(starts[i]), threads=1, public_values=pv)
            assert e.value.status == INVALID_ARG
            w = None
        else:
            w, _cfg = gpu.p3_prove_air(air, t, num_queries=4, pow_bits=8, pow_start=int(starts[i]), threads=1, public_values=pv)
        traces.append(t)
        pvs.append(pv)
        rows.append(w)
    rows[2] = np.zeros_like(rows[0])
    out = (air, np.stack(traces), np.stack(pvs), starts, np.stack(rows))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _two_proof_budget(pr, fib5):
    """A scratch budget under which a group holds exactly two proofs: twice what a one-proof call made the handle hold."""
    _air, traces, pvs, starts, want = fib5
    one, st = pr.prove(traces[:1], public_values=pvs[:1], pow_starts=starts[:1])
    assert st.tolist() == [OK] and np.array_equal(one[0], want[0])
    per_proof = pr.scratch_bytes()[0]
    assert per_proof > 0
    return 2 * per_proof + per_proof // 2


def test_batch_default_budget_and_groups_of_two(gpu, fib5):
    air, traces, pvs, starts, want = fib5
    pr = gpu.P3Prover(air, 3, 1, 4, 8)
    got, st = pr.prove(traces, public_values=pvs, pow_starts=starts)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(got, want) and not got[2].any()
    pr.close()
    pr = gpu.P3Prover(air, 3, 1, 4, 8)
    budget = _two_proof_budget(pr, fib5)
    pr.set_scratch_budget(budget)
    grouped, st = pr.prove(traces, public_values=pvs, pow_starts=starts)          # groups (0, 1), (2, 3), (4)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(grouped, want), np.nonzero((grouped != want).any(axis=1))[0]
    assert budget * 2 // 5 < pr.scratch_bytes()[0] <= budget                      # two proofs' worth, not one, not five
    # another order: every row still goes with its own public values
    order = np.array([4, 0, 3, 1, 2])
    again, st = pr.prove(traces[order], public_values=pvs[order], pow_starts=starts[order])
    assert st.tolist() == [OK, OK, OK, OK, INVALID_ARG] and np.array_equal(again, want[order])
    pr.close()


def _dev_run(pr, traces, pvs, pow_starts, i_stride, stream=0):
    """prove_dev on guard-banded buffers; -> (inputs[n][num_inputs], statuses) after checking every band and the padding."""
    import torch
    n, tw, ni, m = traces.shape[0], traces[0].size, pr.num_inputs, pr.n_public
    d_tr, d_pv, d_ps = Banded(n * tw, before=ODD), Banded(n * m, before=ODD), Banded(n, before=ODD)
    d_in, d_st = Banded(n * i_stride, before=ODD), Banded32(n, before=ODD)
    d_tr.set(np.array(traces).reshape(n, tw))       # copies: the fixtures are read-only
    d_pv.set(np.array(pvs))
    d_ps.set(np.array(pow_starts, dtype=np.uint64))
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.ptr, tw, n, d_ps.ptr, d_in.ptr, i_stride, d_st.ptr, stream, d_public_values=d_pv.ptr)
    pr.sync()
    for b in (d_tr, d_pv, d_ps):
        b.assert_unchanged()
    d_in.assert_bands_intact()
    d_st.assert_bands_intact()
    i_data, i_pad = strided_rows(n, ni, i_stride)
    d_in.assert_untouched(i_pad)
    return d_in.get()[i_data].reshape(n, ni), d_st.get()


@pytest.mark.parametrize("grouped", [False, True])
def test_device_resident_batch_writes_num_inputs_words_per_proof(gpu, fib5, grouped):
    air, traces, pvs, starts, want = fib5
    pr = gpu.P3Prover(air, 3, 1, 4, 8)
    if grouped:
        pr.set_scratch_budget(_two_proof_budget(pr, fib5))
    got, st = _dev_run(pr, traces, pvs, starts, pr.num_inputs + 5)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(got, want)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the verifier
# ---------------------------------------------------------------------------------------------------------------------
def _bumped(words, pos):
    w = np.array(words, dtype=np.uint64)
    w[pos] = (int(w[pos]) + 1) % P
    return w


def mutations(case):
    """name -> proof: a tail word changed (the first, the last), a tail word = p, and one word of every section of the
    proof -- the last query's and the last FRI round's where a section repeats."""
    s, w, m = case.shape, case.words, case.m
    ni, q, r = s.num_inputs, s.queries - 1, s.k - 1
    out = {"tail first": _bumped(w, ni), "tail last": _bumped(w, ni + m - 1)}
    big = np.array(w, dtype=np.uint64)
    big[ni + m // 2] = P
    out["tail word = p"] = big
    places = {"trace root": 0, "quotient root": 5, "trace_local": s.o_trace_local, "trace_next": s.o_trace_next + 1,
              "chunk": s.o_chunks + 2, "fri root": s.o_fri_roots + 4 * r + 3, "fri sibling": s.step(q, r) + 1,
              "fri path": s.step(q, r) + 2 + 4 * (s.L - r - 2) + 1, "final_poly": s.o_final_poly, "pow witness": s.o_pow_witness,
              "trace row": s.opening(q, 0) + s.W - 1, "trace path": s.opening(q, 0) + s.W + 4 * (s.L - 1),
              "quotient row": s.opening(q, 1) + 1, "quotient path": s.opening(q, 1) + 2 * s.Q + 2}
    assert s.L - r - 1 >= 1 and max(places.values()) < ni
    for name, pos in places.items():
        out[name] = _bumped(w, pos)
    return out


@pytest.mark.parametrize("key", CASE_KEYS)
def test_verdicts_equal_the_models(gpu, oracle, key):
    import torch
    case = case_of(gpu, key)
    prover = case.prover(gpu)
    mine, st = prover.prove(case.trace, public_values=case.pv)                       # the device's own proof
    assert st.tolist() == [OK]
    prover.close()
    assert M.verify(oracle, case.air, case.cfg, mine[0]) == M.OK
    muts = mutations(case)
    batch = np.stack([mine[0]] + list(muts.values()))
    want = [M.verify(oracle, case.air, case.cfg, p) for p in batch]
    # a changed public value never passes (it enters alpha and the identity); a changed proof word is the model's to judge
    assert want[0] == M.OK and M.OK not in want[1:4] and want[3] == M.MALFORMED, dict(zip(["untouched"] + list(muts), want))
    pr = case.prover(gpu)                                                            # a handle that only verifies
    got = pr.verify(batch)
    assert got.tolist() == want, [(n, int(g), w) for n, g, w in zip(["untouched"] + list(muts), got, want) if g != w]
    # the device form: a stride above num_inputs, guard bands, nothing but the status words written
    n, ni, stride = batch.shape[0], pr.num_inputs, pr.num_inputs + 3
    d_in, d_st = Banded(n * stride, before=ODD), Banded32(n, before=ODD)
    data, _pad = strided_rows(n, ni, stride)
    interior = d_in.get()
    interior[data] = batch.ravel()
    d_in.set(interior)
    torch.cuda.synchronize()
    pr.verify_dev(d_in.ptr, n, stride, d_st.ptr)
    pr.sync()
    d_in.assert_unchanged()
    d_st.assert_bands_intact()
    assert d_st.get().tolist() == want
    assert pr.scratch_bytes()[0] == 0 and pr.scratch_bytes()[1] > 0                  # no proving scratch
    pr.close()


def test_verifier_accepts_the_batch_of_case_2(gpu, oracle, fib5):
    import torch
    air, traces, pvs, starts, want = fib5
    pr = gpu.P3Prover(air, 3, 1, 4, 8)
    expect = [M.verify(oracle, air, pr.config, row) for row in want]
    assert expect == [M.OK, M.OK, expect[2], M.OK, M.OK] and expect[2] != M.OK        # the zero row of the failed proof
    assert pr.verify(want).tolist() == expect
    d_in, d_st = Banded(want.size, before=ODD), Banded32(5, before=ODD)
    d_in.set(np.array(want))
    torch.cuda.synchronize()
    pr.verify_dev(d_in.ptr, 5, want.shape[1], d_st.ptr)
    pr.sync()
    d_in.assert_unchanged()
    d_st.assert_bands_intact()
    assert d_st.get().tolist() == expect
    # proof 0's words with proof 1's public values: valid words, the wrong statement
    crossed = np.array(want[0])
    crossed[-3:] = want[1][-3:]
    code = M.verify(oracle, air, pr.config, crossed)
    assert code != M.OK and pr.verify(crossed).tolist() == [code]
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the outer proof, 5. aggregation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outer(gpu, oracle):
    """fib_pv at log_n 3, 3 queries, 4 PoW bits: the inner prover, its verifier circuit (3 public inputs), the oracle's
    copy of it from the exported blob, and three inner proofs with different public values."""
    air = air_cases_pv.fib_pv(gpu)
    pr = gpu.P3Prover(air, 3, 1, 3, 4)
    tp = [air_cases_pv.fib_pv_trace(3, a, b) for a, b in ((1, 1), (5, 9), (P - 2, 1 << 50))]
    traces, pvs = np.stack([t for t, _ in tp]), np.stack([v for _, v in tp])
    inner, st = pr.prove(traces, public_values=pvs)
    assert st.tolist() == [OK] * 3
    circuit = gpu.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(circuit.info.num_public_inputs) == 3 and int(circuit.info.num_inputs) == pr.num_inputs
    oc = oracle.load_circuit(circuit.to_blob())
    proofs, st = circuit.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [OK] * 3
    yield pr, circuit, oc, traces, pvs, inner, proofs
    pr.close()


def test_outer_proofs_equal_the_oracles_and_end_in_the_public_values(gpu, outer):
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    dg, cap = circuit.digest()
    for i in range(3):
        po, sto, _tm, msg = oc.prove(inner[i], seed=i + 1)
        assert sto == 0, msg
        assert np.array_equal(proofs[i], po), f"outer proof {i} differs from the oracle's"
        assert proofs[i][-3:].tolist() == pvs[i].tolist() == circuit.public_inputs(proofs[i]).tolist()
        assert oc.verify(proofs[i], dg, cap)[0] == 0
    assert circuit.verify(proofs).tolist() == [OK] * 3


def test_a_changed_public_value_is_a_witness_conflict(gpu, outer):
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    fourth = np.array(inner[1])
    fourth[-2] = (int(fourth[-2]) + 1) % P                                           # pv1 of a valid inner proof
    assert pr.verify(fourth)[0] != OK                                                # the screen sees it too
    got, st = circuit.prove(np.stack([inner[0], inner[1], inner[2], fourth]), seeds=[1, 2, 3, 4])
    assert st.tolist() == [OK, OK, OK, WITNESS_CONFLICT]
    assert np.array_equal(got[:3], proofs)


def test_chain_on_one_stream(gpu, outer):
    """p25_p3_prove_batch_pv_dev -> p25_p3_verify_batch_dev -> p25_circuit_wait_stream -> p25_prove_batch_dev, no host copy."""
    import torch
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    dev = torch.device("cuda", 0)
    n, ni, pw = 3, pr.num_inputs, int(circuit.info.proof_words)
    d_tr = torch.from_numpy(traces.reshape(n, -1).view(np.int64).copy()).to(dev)
    d_pv = torch.from_numpy(pvs.view(np.int64).copy()).to(dev)
    d_seeds = torch.tensor([1, 2, 3], dtype=torch.int64, device=dev)
    d_inputs, d_ist, d_vst = Banded(n * ni), Banded32(n), Banded32(n)
    d_proofs, d_pst = Banded(n * pw), Banded32(n)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.data_ptr(), traces[0].size, n, 0, d_inputs.ptr, ni, d_ist.ptr, side.cuda_stream, d_public_values=d_pv.data_ptr())
    pr.verify_dev(d_inputs.ptr, n, ni, d_vst.ptr, side.cuda_stream)
    circuit.wait_stream(side.cuda_stream)
    circuit.prove_dev(d_inputs.ptr, n, d_seeds.data_ptr(), d_proofs.ptr, pw, d_pst.ptr)
    circuit.sync()
    side.synchronize()
    assert d_ist.get().tolist() == [OK] * 3 and d_vst.get().tolist() == [OK] * 3 and d_pst.get().tolist() == [OK] * 3
    assert np.array_equal(d_inputs.get().reshape(n, ni), inner)
    assert np.array_equal(d_proofs.get().reshape(n, pw), proofs)
    for b in (d_inputs, d_ist, d_vst, d_proofs, d_pst):
        b.assert_bands_intact()


def test_aggregate_commits_to_the_public_values(gpu, oracle, outer):
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    agg = circuit.build_aggregator(2)
    assert int(agg.info.num_public_inputs) == 4
    root, st = agg.prove(np.concatenate([proofs[0], proofs[2]])[None, :], seeds=[9])
    assert st.tolist() == [OK]
    want = oracle.hash_no_pad(np.concatenate([pvs[0], pvs[2]]))
    assert np.array_equal(agg.public_inputs(root[0]), want)
    oa = oracle.load_circuit(agg.to_blob())
    dg, cap = agg.digest()
    assert oa.verify(root[0], dg, cap)[0] == 0
