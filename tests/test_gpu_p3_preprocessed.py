"""GPU: preprocessed columns of the inner STARK on the device (include/p25.h, "PREPROCESSED COLUMNS"): the handle's constant
tables (coefficients, LDE, tree) made once on the device, the prover's kernels reading them beside every proof's own
buffers, the device verifier's third batch, and the outer proof of the verifier circuit.  Field arithmetic is exact: every
comparison is equality.

1. the device prover's words are the host prover's, for each shape of air_cases_preprocessed.SHAPES
2. the handle's commitment is p25_p3_preprocessed_commit's, from a handle that has done nothing else and from one that proved
3. five proofs in groups of two equal the lone proofs: a shared pointer advanced per group would show here
4. the device-resident form with stride padding writes num_inputs words per proof
5. a trace that fails the AIR fails its own proof only; its words are zeros
6. the verifier's verdicts equal the independent model's (tests/p3_preprocessed_model.py): the valid proof, single-word flips
   in every new region of every query, and a handle whose columns differ in one cell
7. a handle that only verifies holds no proving scratch -- not the tables either
8. chunks change no verdict
9. prove -> verify -> outer prove on one stream
10. outer proofs equal the oracle's"""
import numpy as np
import pytest

import air_cases_preprocessed as cases
import p3_preprocessed_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097
QUERIES, POW_BITS = 4, 8


class Case:
    """A shape of air_cases_preprocessed.SHAPES: the AIR, one satisfying trace, the HOST prover's flat proof of it and the
    host's commitment of the columns."""

    def __init__(self, p25, shape):
        self.air, self.trace, self.pv, self.prep, self.log_n, self.log_blowup = cases.make(p25, shape)
        self.words, self.cfg = p25.p3_prove_air(self.air, self.trace, num_queries=QUERIES, pow_bits=POW_BITS,
                                                log_blowup=self.log_blowup, threads=1, public_values=self.pv)
        self.pw = self.prep.shape[1]
        self.shape = M.Shape(self.cfg, self.pw)
        self.commit = p25.p3_preprocessed_commit(self.prep, self.log_blowup, threads=1)
        assert self.words.size == self.shape.num_inputs + self.air.n_public
        self.words.setflags(write=False)

    def prover(self, p25, air=None):
        return p25.P3Prover(air or self.air, self.log_n, self.log_blowup, QUERIES, POW_BITS)


_cases = {}


def case_of(p25, shape):
    if shape[0] not in _cases:
        _cases[shape[0]] = Case(p25, shape)
    return _cases[shape[0]]


def _bumped(words, pos):
    w = np.array(words, dtype=np.uint64)
    w[pos] = (int(w[pos]) + 1) % P
    return w


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2, 5. device == host, word for word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_device_words_are_the_host_words(gpu, shape):
    case = case_of(gpu, shape)
    pr = case.prover(gpu)
    assert pr.num_inputs == case.words.size and bytes(pr.config) == bytes(case.cfg)
    got, st = pr.prove(case.trace, public_values=case.pv)
    assert st.tolist() == [OK]
    assert np.array_equal(got[0], case.words), np.nonzero(got[0] != case.words)[0][:8]
    assert pr.preprocessed_commit().tolist() == case.commit.tolist()              # the tables' root, after proving
    # a cell of the trace changed: this proof fails in the identity kernel, its row is zeros
    bad = case.trace.copy()
    r = (1 << case.log_n) - 2
    bad[r, -1] = (int(bad[r, -1]) + 1) % P
    got, st = pr.prove(bad, public_values=case.pv)
    assert st.tolist() == [INVALID_ARG] and not got.any()
    pr.close()


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_a_fresh_handles_commitment_is_the_hosts(gpu, shape):
    """No compute call before it: the handle makes the tables in a temporary, keeps the 4 words and no scratch."""
    case = case_of(gpu, shape)
    pr = case.prover(gpu)
    assert pr.preprocessed_commit().tolist() == case.commit.tolist()
    assert pr.preprocessed_commit().tolist() == case.commit.tolist()
    assert pr.scratch_bytes() == (0, 0)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4, 5. a batch with groups
# ---------------------------------------------------------------------------------------------------------------------
FIVE = "machine3"


@pytest.fixture(scope="module")
def five(gpu):
    """Five prep_machine(3) instances under the same columns with distinct public values; proof 2's trace has one cell
    changed.  -> (air, traces[5], pvs[5][2], pow_starts, host rows[5] with row 2 zeros)."""
    shp = cases.shape(FIVE)
    traces, pvs, rows = [], [], []
    starts = np.array([0, 1 << 20, 5, 7 << 30, 3], dtype=np.uint64)
    for i in range(5):
        air, t, pv, _prep, _log_n, log_blowup = cases.make(gpu, shp, x0=100 + 7 * i)
        if i == 2:
            t[5, 0] = (int(t[5, 0]) + 1) % P
        prove = lambda: gpu.p3_prove_air(air, t, num_queries=QUERIES, pow_bits=POW_BITS, pow_start=int(starts[i]), threads=1,  # noqa: E731
                                         log_blowup=log_blowup, public_values=pv)
        if i == 2:
            with pytest.raises(gpu.P25Error) as e:
                prove()
            assert e.value.status == INVALID_ARG
            w = None
        else:
            w, _cfg = prove()
        traces.append(t)
        pvs.append(pv)
        rows.append(w)
    rows[2] = np.zeros_like(rows[0])
    out = (air, np.stack(traces), np.stack(pvs), starts, np.stack(rows))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _prover5(gpu, air):
    _id, _kind, _args, log_n, log_blowup = cases.shape(FIVE)
    return gpu.P3Prover(air, log_n, log_blowup, QUERIES, POW_BITS)


def _table_bytes(pr):
    """The preprocessed tables of a handle: coefficients PW n, LDE PW N2, tree 8 N2 words (include/p25.h)."""
    _id, _kind, _args, log_n, log_blowup = cases.shape(FIVE)
    n, n2 = 1 << log_n, 1 << (log_n + log_blowup)
    return 8 * (2 * n + 2 * n2 + 8 * n2)


def _two_proof_budget(pr, five):
    """A scratch budget under which a group holds exactly two proofs.  scratch_bytes counts the tables under `proving`; the
    budget does not."""
    _air, traces, pvs, starts, want = five
    one, st = pr.prove(traces[:1], public_values=pvs[:1], pow_starts=starts[:1])
    assert st.tolist() == [OK] and np.array_equal(one[0], want[0])
    per_proof = pr.scratch_bytes()[0] - _table_bytes(pr)
    assert per_proof > 0
    return 2 * per_proof + per_proof // 2


def test_batch_default_budget_and_groups_of_two(gpu, five):
    air, traces, pvs, starts, want = five
    pr = _prover5(gpu, air)
    got, st = pr.prove(traces, public_values=pvs, pow_starts=starts)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(got, want) and not got[2].any()
    pr.close()
    pr = _prover5(gpu, air)
    budget = _two_proof_budget(pr, five)
    pr.set_scratch_budget(budget)
    grouped, st = pr.prove(traces, public_values=pvs, pow_starts=starts)          # groups (0, 1), (2, 3), (4)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(grouped, want), np.nonzero((grouped != want).any(axis=1))[0]
    held = pr.scratch_bytes()[0] - _table_bytes(pr)
    assert budget * 2 // 5 < held <= budget                                       # two proofs' worth, not one, not five
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
def test_device_resident_batch_writes_num_inputs_words_per_proof(gpu, five, grouped):
    air, traces, pvs, starts, want = five
    pr = _prover5(gpu, air)
    if grouped:
        pr.set_scratch_budget(_two_proof_budget(pr, five))
    got, st = _dev_run(pr, traces, pvs, starts, pr.num_inputs + 5)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(got, want)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6, 7. the verifier
# ---------------------------------------------------------------------------------------------------------------------
def mutations(case):
    """name -> proof: single-word flips that cover every region preprocessed columns add -- the first and the last word of
    both openings and, for EVERY query, of the third batch's row and of its path -- and one word of every older section."""
    s, w = case.shape, case.words
    q, r = s.queries - 1, s.k - 1
    places = {"trace root": 0, "quotient root": 5, "trace_local": s.o_trace_local, "trace_next": s.o_trace_next + 1,
              "chunk": s.o_chunks + 2, "fri root": s.o_fri_roots + 4 * r + 3, "fri sibling": s.step(q, r) + 1,
              "final_poly": s.o_final_poly, "pow witness": s.o_pow_witness, "trace row": s.opening(q, 0) + s.W - 1,
              "trace path": s.opening(q, 0) + s.W + 4 * (s.L - 1), "quotient row": s.opening(q, 1) + 1,
              "quotient path": s.opening(q, 1) + 2 * s.Q + 2}
    for name, ranges in M.regions(case.cfg, case.pw).items():
        for i, (lo, hi) in enumerate(ranges):
            places["%s %d first" % (name, i)] = lo
            places["%s %d last" % (name, i)] = hi - 1
    assert max(places.values()) < s.num_inputs
    return {name: _bumped(w, pos) for name, pos in places.items()}


def _one_cell_changed(case):
    other = case.prep.copy()
    r, c = other.shape[0] // 2, other.shape[1] - 1
    other[r, c] = (int(other[r, c]) + 1) % P
    return other


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
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
    assert want[0] == M.OK, dict(zip(names, want))                                  # a changed word is the model's to judge
    new = [w for n, w in zip(names, want) if n.startswith(("row", "path"))]
    assert new and set(new) == {M.INPUT_MERKLE}                                     # the third batch fails as an input batch (32)
    pr = case.prover(gpu)                                                            # a handle that only verifies
    got = pr.verify(batch)
    assert got.tolist() == want, [(n, int(g), w) for n, g, w in zip(names, got, want) if g != w]
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
    assert pr.scratch_bytes()[0] == 0 and pr.scratch_bytes()[1] > 0                  # no proving scratch, no tables
    pr.close()
    # a handle whose columns differ in one cell: another key.  The model under that key says what fails first.
    other = _one_cell_changed(case)
    other_air = cases.make(gpu, shape, prep=other)[0]
    other_commit = gpu.p3_preprocessed_commit(other, case.log_blowup, threads=1)
    expect = M.verify(oracle, other_air, case.cfg, mine[0], other_commit)
    assert expect != M.OK
    po = case.prover(gpu, other_air)
    assert po.verify(np.stack([mine[0], mine[0]])).tolist() == [expect, expect]
    po.close()


def test_verify_only_takes_no_proving_scratch(gpu, oracle):
    import torch
    case = case_of(gpu, cases.shape("mix64"))
    pr = case.prover(gpu)
    assert pr.scratch_bytes() == (0, 0)
    torch.cuda.synchronize()
    batch = np.stack([case.words] * 3 + [_bumped(case.words, case.shape.opening(1, 2))])
    assert pr.verify(batch).tolist() == [OK, OK, OK, M.INPUT_MERKLE]
    proving, verifying = pr.scratch_bytes()
    k = case.log_n
    assert proving == 0 and verifying == 4 * (8 + 2 * k + QUERIES + 2 * QUERIES * k) * 8
    assert pr.preprocessed_commit().tolist() == case.commit.tolist() and pr.scratch_bytes()[0] == 0
    pr.close()


def test_chunks_change_no_verdict(gpu, oracle):
    case = case_of(gpu, cases.shape("machine2"))
    muts = mutations(case)
    batch = np.stack([case.words] + list(muts.values()))
    want = [M.verify(oracle, case.air, case.cfg, p, case.commit) for p in batch]
    assert want[0] == M.OK
    pr = case.prover(gpu)
    k = case.log_n
    per_proof = (8 + 2 * k + QUERIES + 2 * QUERIES * k) * 8
    for budget in (1, 5 * per_proof, 7 * per_proof + 8):
        pr.set_scratch_budget(budget)
        assert pr.verify(batch).tolist() == want, budget
    assert pr.scratch_bytes() == (0, 7 * per_proof)          # grown to the largest chunk, never to the batch
    pr.set_scratch_budget(0)
    assert pr.verify(batch[::-1].copy()).tolist() == want[::-1]
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9, 10. the outer proof
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outer(gpu, oracle):
    """prep_machine(3) at log_n 3, 3 queries, 4 PoW bits: the inner prover, its verifier circuit, the oracle's copy of it from
    the exported blob, three inner proofs with different public values and their outer proofs."""
    shp = cases.shape(FIVE)
    made = [cases.make(gpu, shp, x0=x0) for x0 in (1, 11, P - 2)]
    air, log_n, log_blowup = made[0][0], made[0][4], made[0][5]
    pr = gpu.P3Prover(air, log_n, log_blowup, 3, 4)
    traces, pvs = np.stack([m[1] for m in made]), np.stack([m[2] for m in made])
    inner, st = pr.prove(traces, public_values=pvs)
    assert st.tolist() == [OK] * 3
    circuit = gpu.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(circuit.info.num_public_inputs) == 2 and int(circuit.info.num_inputs) == pr.num_inputs
    oc = oracle.load_circuit(circuit.to_blob())
    proofs, st = circuit.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [OK] * 3
    yield pr, circuit, oc, traces, pvs, inner, proofs, made[0][3]
    pr.close()


def test_outer_proofs_equal_the_oracles(gpu, outer):
    pr, circuit, oc, traces, pvs, inner, proofs, prep = outer
    dg, cap = circuit.digest()
    for i in range(3):
        po, sto, _tm, msg = oc.prove(inner[i], seed=i + 1)
        assert sto == 0, msg
        assert np.array_equal(proofs[i], po), f"outer proof {i} differs from the oracle's"
        assert proofs[i][-2:].tolist() == pvs[i].tolist()
        assert oc.verify(proofs[i], dg, cap)[0] == 0
    assert circuit.verify(proofs).tolist() == [OK] * 3


def test_a_circuit_for_other_columns_is_a_witness_conflict(gpu, outer):
    pr, circuit, oc, traces, pvs, inner, proofs, prep = outer
    other = prep.copy()
    other[3, 1] = (int(other[3, 1]) + 1) % P
    other_air = cases.make(gpu, cases.shape(FIVE), prep=other)[0]
    c2 = gpu.Circuit.build_p3_verifier_air(pr.config, other_air)
    assert c2.digest()[0].tolist() != circuit.digest()[0].tolist()
    got, st = c2.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [WITNESS_CONFLICT] * 3


def test_chain_on_one_stream(gpu, outer):
    """p25_p3_prove_batch_pv_dev -> p25_p3_verify_batch_dev -> p25_circuit_wait_stream -> p25_prove_batch_dev, no host copy."""
    import torch
    pr, circuit, oc, traces, pvs, inner, proofs, prep = outer
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
