"""GPU: challenges and auxiliary running-sum columns of the inner STARK on the device (include/p25.h, "AUXILIARY COLUMNS"):
the chain's challenge phase, the term kernel with its one inversion per row, the three-launch prefix sum in F_p^2, the fourth
commit, the quotient in F_p^2, the device verifier's fourth batch, and the outer proof of the verifier circuit.  Field
arithmetic is exact: every comparison is equality.

1. the device prover's words are the host prover's, for each shape and height of air_cases_aux
2. a bad trace (no permutation, a wrong multiplicity, a zero denominator) fails its own proof only, with zero words
3. five proofs in groups of two equal the lone proofs; proof 2 is no permutation, proof 3 has a zero denominator
4. the device-resident form on guard-banded, stride-padded buffers
5. the verifier's verdicts equal the independent model's (tests/p3_aux_model.py) on single-word flips in every new region
   of every query, and for a handle made for another num node
6. a handle that only verifies reports proving_out == 0
7. chunks change no verdict
8. prove -> verify -> outer prove on one stream; outer proofs equal the oracle's
9. a circuit built for another AIR gives P25_ERR_WITNESS_CONFLICT"""
import numpy as np
import pytest

import air_cases_aux as cases
import p3_aux_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097
QUERIES, POW_BITS = 4, 8


class Case:
    """A shape of air_cases_aux: the AIR, one satisfying trace and the HOST prover's flat proof of it."""

    def __init__(self, p25, shape, queries=QUERIES, pow_bits=POW_BITS, threads=1):
        self.air, self.trace, self.pv, self.log_n, self.log_blowup = cases.make(p25, shape)
        self.queries, self.pow_bits = queries, pow_bits
        self.words, self.cfg = p25.p3_prove_air(self.air, self.trace, num_queries=queries, pow_bits=pow_bits,
                                                log_blowup=self.log_blowup, threads=threads, public_values=self.pv)
        self.pw = 0 if self.air.preprocessed is None else int(self.air.preprocessed.shape[1])
        self.aw = len(self.air.aux_columns)
        self.commit = None if not self.pw else p25.p3_preprocessed_commit(self.air.preprocessed, self.log_blowup, threads=1)
        self.shape = M.Shape(self.cfg, self.pw, self.aw)
        assert self.words.size == self.shape.num_inputs + self.air.n_public
        self.words.setflags(write=False)

    def prover(self, p25, air=None):
        return p25.P3Prover(air or self.air, self.log_n, self.log_blowup, self.queries, self.pow_bits)


_cases = {}


def case_of(p25, shape):
    if shape[0] not in _cases:
        _cases[shape[0]] = Case(p25, shape)
    return _cases[shape[0]]


def _bumped(words, pos):
    w = np.array(words, dtype=np.uint64)
    w[pos] = (int(w[pos]) + 1) % P
    return w


def _bad_trace(case):
    """A trace that breaks the multiset argument: one cell of the last column changed."""
    bad = case.trace.copy()
    r = (1 << case.log_n) // 2
    bad[r, -1] = (int(bad[r, -1]) + 1) % P
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. device == host, word for word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_device_words_are_the_host_words(gpu, shape):
    case = case_of(gpu, shape)
    pr = case.prover(gpu)
    assert pr.num_inputs == case.words.size and bytes(pr.config) == bytes(case.cfg)
    got, st = pr.prove(case.trace, public_values=case.pv)
    assert st.tolist() == [OK]
    assert np.array_equal(got[0], case.words), np.nonzero(got[0] != case.words)[0][:8]
    assert pr.aux_stage_ms() > 0                                                 # the challenge phase ran, between its events
    got, st = pr.prove(_bad_trace(case), public_values=case.pv)                  # fails in the identity kernel: zeros
    assert st.tolist() == [INVALID_ARG] and not got.any()
    pr.close()


@pytest.mark.parametrize("shape", cases.BIG_SHAPES, ids=cases.BIG_IDS)
def test_device_words_are_the_host_words_where_the_totals_take_a_second_tile(gpu, shape):
    """2 queries, no proof of work, 16 host threads: the heights on either side of the totals pass's second tile."""
    case = Case(gpu, shape, queries=2, pow_bits=0, threads=16)
    pr = case.prover(gpu)
    got, st = pr.prove(case.trace)
    assert st.tolist() == [OK]
    assert np.array_equal(got[0], case.words), np.nonzero(got[0] != case.words)[0][:8]
    pr.close()


@pytest.mark.parametrize("row", [0, 5, 7])
def test_a_zero_denominator_fails_the_proof_with_zero_words(gpu, row):
    case = case_of(gpu, cases.shape("det"))
    bad = case.trace.copy()
    bad[row, 1] = 0
    pr = case.prover(gpu)
    got, st = pr.prove(np.stack([case.trace, bad, case.trace]))
    assert st.tolist() == [OK, INVALID_ARG, OK]
    assert np.array_equal(got[0], case.words) and not got[1].any() and np.array_equal(got[2], case.words)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4. a batch with groups
# ---------------------------------------------------------------------------------------------------------------------
FIVE = "tuple"


def _five_air(gpu):
    """The tuple AIR (2 challenges, AW = 2) with a third column whose denominator is trace column 4 + 1: a multiplicity of
    p - 1 there is a zero denominator whatever the challenges are."""
    air = cases.tuple_air(gpu)
    num = air.const(0)
    den = air.add(air.local(4), air.const(1))
    j = air.aux_column(num, den)
    cases._running_sum_constraints(air, j, num, den)
    return air


@pytest.fixture(scope="module")
def five(gpu):
    """Five instances; proof 2's pairs are not in the table (the terms do not sum to zero), proof 3 has a zero denominator.
    -> (air, traces[5], pow_starts, host rows[5] with rows 2 and 3 zeros)."""
    _id, _kind, _arg, log_n, log_blowup = cases.shape(FIVE)
    air = _five_air(gpu)
    traces, rows = [], []
    starts = np.array([0, 1 << 20, 5, 7 << 30, 3], dtype=np.uint64)
    for i in range(5):
        t = cases.tuple_trace(log_n, seed=i)
        if i == 2:
            t[3, 0] = (int(t[3, 0]) + 1) % P
        if i == 3:
            t[6, 4] = P - 1
        prove = lambda: gpu.p3_prove_air(air, t, num_queries=QUERIES, pow_bits=POW_BITS, pow_start=int(starts[i]), threads=1,  # noqa: E731
                                         log_blowup=log_blowup)
        if i in (2, 3):
            with pytest.raises(gpu.P25Error) as e:
                prove()
            assert e.value.status == INVALID_ARG and ("zero denominator" in str(e.value)) == (i == 3)
            w = None
        else:
            w, _cfg = prove()
        traces.append(t)
        rows.append(w)
    rows[2] = rows[3] = np.zeros_like(rows[0])
    out = (air, np.stack(traces), starts, np.stack(rows))
    for a in out[1:]:
        a.setflags(write=False)
    return out


STATUS5 = [OK, OK, INVALID_ARG, INVALID_ARG, OK]


def _prover5(gpu, air):
    _id, _kind, _arg, log_n, log_blowup = cases.shape(FIVE)
    return gpu.P3Prover(air, log_n, log_blowup, QUERIES, POW_BITS)


def _two_proof_budget(pr, five):
    _air, traces, starts, want = five
    one, st = pr.prove(traces[:1], pow_starts=starts[:1])
    assert st.tolist() == [OK] and np.array_equal(one[0], want[0])
    per_proof = pr.scratch_bytes()[0]
    assert per_proof > 0
    return 2 * per_proof + per_proof // 2


def test_batch_default_budget_and_groups_of_two(gpu, five):
    air, traces, starts, want = five
    pr = _prover5(gpu, air)
    got, st = pr.prove(traces, pow_starts=starts)
    assert st.tolist() == STATUS5
    assert np.array_equal(got, want)
    pr.close()
    pr = _prover5(gpu, air)
    budget = _two_proof_budget(pr, five)
    pr.set_scratch_budget(budget)
    grouped, st = pr.prove(traces, pow_starts=starts)                             # groups (0, 1), (2, 3), (4)
    assert st.tolist() == STATUS5
    assert np.array_equal(grouped, want), np.nonzero((grouped != want).any(axis=1))[0]
    assert budget * 2 // 5 < pr.scratch_bytes()[0] <= budget                      # two proofs' worth, not one, not five
    order = np.array([4, 0, 3, 1, 2])
    again, st = pr.prove(traces[order], pow_starts=starts[order])
    assert st.tolist() == [STATUS5[i] for i in order] and np.array_equal(again, want[order])
    pr.close()


@pytest.mark.parametrize("grouped", [False, True])
def test_device_resident_batch_writes_num_inputs_words_per_proof(gpu, five, grouped):
    import torch
    air, traces, starts, want = five
    pr = _prover5(gpu, air)
    if grouped:
        pr.set_scratch_budget(_two_proof_budget(pr, five))
    n, tw, ni = traces.shape[0], traces[0].size, pr.num_inputs
    i_stride, t_stride = ni + 5, tw + 3
    d_tr, d_ps = Banded(n * t_stride, before=ODD), Banded(n, before=ODD)
    d_in, d_st = Banded(n * i_stride, before=ODD), Banded32(n, before=ODD)
    t_data, _t_pad = strided_rows(n, tw, t_stride)
    interior = d_tr.get()
    interior[t_data] = np.array(traces).reshape(-1)
    d_tr.set(interior)
    d_ps.set(np.array(starts, dtype=np.uint64))
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.ptr, t_stride, n, d_ps.ptr, d_in.ptr, i_stride, d_st.ptr)
    pr.sync()
    for b in (d_tr, d_ps):
        b.assert_unchanged()
    d_in.assert_bands_intact()
    d_st.assert_bands_intact()
    i_data, i_pad = strided_rows(n, ni, i_stride)
    d_in.assert_untouched(i_pad)
    assert d_st.get().tolist() == STATUS5
    assert np.array_equal(d_in.get()[i_data].reshape(n, ni), want)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5, 6, 7. the verifier
# ---------------------------------------------------------------------------------------------------------------------
def mutations(case):
    """name -> proof: single-word flips that cover every region auxiliary columns add -- the first and the last word of the
    commitment and of both openings and, for EVERY query, of the last batch's row and of its path -- and one word of every
    older section."""
    s, w = case.shape, case.words
    q, r = s.queries - 1, s.k - 1
    places = {"trace root": 0, "quotient root": 5, "trace_local": s.o_trace_local, "trace_next": s.o_trace_next + 1,
              "chunk": s.o_chunks + 2, "fri root": s.o_fri_roots + 4 * r + 3, "fri sibling": s.step(q, r) + 1,
              "final_poly": s.o_final_poly, "pow witness": s.o_pow_witness, "trace row": s.opening(q, 0) + s.W - 1,
              "trace path": s.opening(q, 0) + s.W + 4 * (s.L - 1), "quotient row": s.opening(q, 1) + 1,
              "quotient path": s.opening(q, 1) + 2 * s.Q + 2}
    if case.pw:
        places["prep row"] = s.opening(q, 2)
        places["prep path"] = s.opening(q, 2) + case.pw + 1
    for name, ranges in M.regions(case.cfg, case.pw, case.aw).items():
        for i, (lo, hi) in enumerate(ranges):
            places["%s %d first" % (name, i)] = lo
            places["%s %d last" % (name, i)] = hi - 1
    assert max(places.values()) < s.num_inputs
    return {name: _bumped(w, pos) for name, pos in places.items()}


@pytest.mark.parametrize("shape", cases.SHAPES[:8], ids=cases.SHAPE_IDS[:8])
def test_verdicts_equal_the_models(gpu, oracle, shape):
    import torch
    case = case_of(gpu, shape)
    prover = case.prover(gpu)
    mine, st = prover.prove(case.trace, public_values=case.pv)                       # the device's own proof
    assert st.tolist() == [OK]
    prover.close()
    muts = mutations(case)
    names = ["untouched"] + list(muts)
    batch = np.stack([mine[0]] + list(muts.values()))
    want = [M.verify(oracle, case.air, case.cfg, p, case.commit) for p in batch]
    assert want[0] == M.OK, dict(zip(names, want))
    new = [w for n, w in zip(names, want) if n.startswith(("row", "path"))]
    assert new and set(new) == {M.INPUT_MERKLE}                                     # the last batch fails as an input batch (32)
    pr = case.prover(gpu)                                                            # a handle that only verifies
    got = pr.verify(batch)
    assert got.tolist() == want, [(n, int(g), w) for n, g, w in zip(names, got, want) if g != w]
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
    proving, verifying = pr.scratch_bytes()
    k = case.log_n
    nc = case.air.n_challenges
    assert proving == 0                                                              # a verify-only handle: no proving scratch
    assert verifying == n * (8 + 2 * k + QUERIES + 2 * nc + 2 * QUERIES * k) * 8     # the challenge block grows by 2 NC words
    pr.close()


def test_a_handle_for_another_num_node_rejects(gpu, oracle):
    case = case_of(gpu, cases.shape("perm"))
    other = gpu.Air(2, aux=1)
    a, b, g = other.local(0), other.local(1), other.challenge(0)
    num, den = a, other.mul(other.sub(g, a), other.sub(g, b))                        # num = a, not a - b
    other.aux_column(num, den)
    cases._running_sum_constraints(other, 0, num, den)
    expect = M.verify(oracle, other, case.cfg, case.words)
    assert expect == M.CONSTRAINTS
    po = case.prover(gpu, other)
    assert po.verify(np.stack([case.words, case.words])).tolist() == [expect, expect]
    got, st = po.prove(case.trace)                                                   # and it cannot prove the permutation
    assert st.tolist() == [INVALID_ARG] and not got.any()
    po.close()


def test_chunks_change_no_verdict(gpu, oracle):
    case = case_of(gpu, cases.shape("range"))
    muts = mutations(case)
    batch = np.stack([case.words] + list(muts.values()))
    want = [M.verify(oracle, case.air, case.cfg, p, case.commit) for p in batch]
    assert want[0] == M.OK
    pr = case.prover(gpu)
    k = case.log_n
    per_proof = (8 + 2 * k + QUERIES + 2 * case.air.n_challenges + 2 * QUERIES * k) * 8
    for budget in (1, 5 * per_proof, 7 * per_proof + 8):
        pr.set_scratch_budget(budget)
        assert pr.verify(batch).tolist() == want, budget
    assert pr.scratch_bytes() == (0, 7 * per_proof)          # grown to the largest chunk, never to the batch
    pr.set_scratch_budget(0)
    assert pr.verify(batch[::-1].copy()).tolist() == want[::-1]
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8, 9. the outer proof
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outer(gpu, oracle):
    """The range lookup (auxiliary beside preprocessed columns) at 3 queries, 4 PoW bits: the inner prover, its verifier
    circuit, the oracle's copy of it from the exported blob, three inner proofs and their outer proofs."""
    shp = cases.shape("range")
    made = [cases.make(gpu, shp, seed=s) for s in (1, 2, 3)]
    air, log_n, log_blowup = made[0][0], made[0][3], made[0][4]
    pr = gpu.P3Prover(air, log_n, log_blowup, 3, 4)
    traces = np.stack([m[1] for m in made])
    inner, st = pr.prove(traces)
    assert st.tolist() == [OK] * 3
    circuit = gpu.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(circuit.info.num_inputs) == pr.num_inputs
    oc = oracle.load_circuit(circuit.to_blob())
    proofs, st = circuit.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [OK] * 3
    yield pr, circuit, oc, traces, inner, proofs
    pr.close()


def test_outer_proofs_equal_the_oracles(gpu, outer):
    pr, circuit, oc, traces, inner, proofs = outer
    dg, cap = circuit.digest()
    for i in range(3):
        po, sto, _tm, msg = oc.prove(inner[i], seed=i + 1)
        assert sto == 0, msg
        assert np.array_equal(proofs[i], po), f"outer proof {i} differs from the oracle's"
        assert oc.verify(proofs[i], dg, cap)[0] == 0
    assert circuit.verify(proofs).tolist() == [OK] * 3


def test_a_circuit_for_another_air_is_a_witness_conflict(gpu, outer):
    pr, circuit, oc, traces, inner, proofs = outer
    log_n = cases.shape("range")[3]
    other = gpu.Air(2, preprocessed=cases.range_table(log_n), aux=1)
    f, m, t, g = other.local(0), other.local(1), other.prep_local(0), other.challenge(0)
    gf, gt = other.sub(g, f), other.sub(g, t)
    num = other.sub(other.mul(m, gf), other.add(gt, other.const(1)))                 # another numerator
    den = other.mul(gt, gf)
    other.aux_column(num, den)
    cases._running_sum_constraints(other, 0, num, den)
    c2 = gpu.Circuit.build_p3_verifier_air(pr.config, other)
    assert c2.digest()[0].tolist() != circuit.digest()[0].tolist()
    got, st = c2.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [WITNESS_CONFLICT] * 3


def test_chain_on_one_stream(gpu, outer):
    """p25_p3_prove_batch_dev -> p25_p3_verify_batch_dev -> p25_circuit_wait_stream -> p25_prove_batch_dev, no host copy."""
    import torch
    pr, circuit, oc, traces, inner, proofs = outer
    dev = torch.device("cuda", 0)
    n, ni, pw = 3, pr.num_inputs, int(circuit.info.proof_words)
    d_tr = torch.from_numpy(traces.reshape(n, -1).view(np.int64).copy()).to(dev)
    d_seeds = torch.tensor([1, 2, 3], dtype=torch.int64, device=dev)
    d_inputs, d_ist, d_vst = Banded(n * ni), Banded32(n), Banded32(n)
    d_proofs, d_pst = Banded(n * pw), Banded32(n)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.data_ptr(), traces[0].size, n, 0, d_inputs.ptr, ni, d_ist.ptr, side.cuda_stream)
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
