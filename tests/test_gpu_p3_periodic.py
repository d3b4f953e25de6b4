"""GPU: periodic columns of the inner STARK on the device (include/p25.h, "PERIODIC COLUMNS"): the device prover reading the
columns' coset tables in k_p3_quotient and evaluating them at zeta in k_p3_identity, the device verifier's identity lane, and
the outer proof of the verifier circuit.  Field arithmetic is exact: every comparison is equality.

1. the device prover's words are the host prover's, for each shape of air_cases_periodic.SHAPES -- among them the ones at
   which the quotient kernel's bit-reversed lane-to-table mapping crosses a block (n Q = 512, 1024) and the caps
2. a batch in groups: the tables are the handle's, shared by every proof of every group; a failed proof is zeros
3. the verifier's verdict equals the independent model's (tests/p3_periodic_model.py) for a mutation of every section, and a
   handle whose columns differ in one value rejects a valid proof for its constraints (35), nothing else
4. the outer proof equals the oracle's; a circuit built with one round constant changed gives a witness conflict; the chain
   prove -> verify -> outer prove on one stream"""
import numpy as np
import pytest

import air_cases_periodic as cases
import p3_periodic_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097
QUERIES, POW_BITS = 4, 8


class Case:
    """A shape of air_cases_periodic.SHAPES: the AIR, one satisfying trace and the HOST prover's flat proof of it."""

    def __init__(self, p25, shape):
        self.air, self.trace, self.pv, self.log_n, self.log_blowup = cases.make(p25, shape)
        self.words, self.cfg = p25.p3_prove_air(self.air, self.trace, num_queries=QUERIES, pow_bits=POW_BITS,
                                                log_blowup=self.log_blowup, threads=1, public_values=self.pv)
        self.shape = M.Shape(self.cfg)
        self.m = self.air.n_public
        assert self.words.size == self.shape.num_inputs + self.m
        self.words.setflags(write=False)

    def prover(self, p25, air=None):
        return p25.P3Prover(air or self.air, self.log_n, self.log_blowup, QUERIES, POW_BITS)


_cases = {}


def case_of(p25, shape):
    if shape[0] not in _cases:
        _cases[shape[0]] = Case(p25, shape)
    return _cases[shape[0]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. device == host, word for word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_device_words_are_the_host_words(gpu, shape):
    case = case_of(gpu, shape)
    pr = case.prover(gpu)
    assert pr.num_inputs == case.words.size and bytes(pr.config) == bytes(case.cfg)
    got, st = pr.prove(case.trace, public_values=case.pv)
    assert st.tolist() == [OK]
    assert np.array_equal(got[0], case.words), np.nonzero(got[0] != case.words)[0][:8]
    # a cell of the trace changed: this proof fails in the identity kernel, its row is zeros
    bad = case.trace.copy()
    r = (1 << case.log_n) - 1
    bad[r, -1] = (int(bad[r, -1]) + 1) % P
    got, st = pr.prove(bad, public_values=case.pv)
    assert st.tolist() == [INVALID_ARG] and not got.any()
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. a batch with groups
# ---------------------------------------------------------------------------------------------------------------------
MIMC5 = (2, 3, 3, 2)          # k, d, log_n, log_blowup


@pytest.fixture(scope="module")
def mimc5(gpu):
    """Five mimc(2, 3) instances with distinct public values; proof 2's trace has one cell changed.
    -> (air, traces[5], pvs[5][2], pow_starts, host rows[5] with row 2 zeros)."""
    k, d, log_n, log_blowup = MIMC5
    air = cases.mimc(gpu, k, d)
    traces, pvs, rows = [], [], []
    starts = np.array([0, 1 << 20, 5, 7 << 30, 3], dtype=np.uint64)
    for i in range(5):
        t, pv = cases.mimc_trace(log_n, k, d, 100 + 7 * i)
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
    k, d, log_n, log_blowup = MIMC5
    return gpu.P3Prover(air, log_n, log_blowup, QUERIES, POW_BITS)


def _two_proof_budget(pr, mimc5):
    """A scratch budget under which a group holds exactly two proofs: twice what a one-proof call made the handle hold."""
    _air, traces, pvs, starts, want = mimc5
    one, st = pr.prove(traces[:1], public_values=pvs[:1], pow_starts=starts[:1])
    assert st.tolist() == [OK] and np.array_equal(one[0], want[0])
    per_proof = pr.scratch_bytes()[0]
    assert per_proof > 0
    return 2 * per_proof + per_proof // 2


def test_batch_default_budget_and_groups_of_two(gpu, mimc5):
    air, traces, pvs, starts, want = mimc5
    pr = _prover5(gpu, air)
    got, st = pr.prove(traces, public_values=pvs, pow_starts=starts)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(got, want) and not got[2].any()
    pr.close()
    pr = _prover5(gpu, air)
    budget = _two_proof_budget(pr, mimc5)
    pr.set_scratch_budget(budget)
    grouped, st = pr.prove(traces, public_values=pvs, pow_starts=starts)          # groups (0, 1), (2, 3), (4)
    assert st.tolist() == [OK, OK, INVALID_ARG, OK, OK]
    assert np.array_equal(grouped, want), np.nonzero((grouped != want).any(axis=1))[0]
    assert budget * 2 // 5 < pr.scratch_bytes()[0] <= budget                      # two proofs' worth, not one, not five
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
def test_device_resident_batch_writes_num_inputs_words_per_proof(gpu, mimc5, grouped):
    air, traces, pvs, starts, want = mimc5
    pr = _prover5(gpu, air)
    if grouped:
        pr.set_scratch_budget(_two_proof_budget(pr, mimc5))
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
    """name -> proof: one word of every section of the proof changed -- the section list of
    test_gpu_p3_public_values.mutations, the last query's and the last FRI round's where a section repeats."""
    s, w = case.shape, case.words
    ni, q, r = s.num_inputs, s.queries - 1, s.k - 1
    places = {"trace root": 0, "quotient root": 5, "trace_local": s.o_trace_local, "trace_next": s.o_trace_next + 1,
              "chunk": s.o_chunks + 2, "fri root": s.o_fri_roots + 4 * r + 3, "fri sibling": s.step(q, r) + 1,
              "fri path": s.step(q, r) + 2 + 4 * (s.L - r - 2) + 1, "final_poly": s.o_final_poly, "pow witness": s.o_pow_witness,
              "trace row": s.opening(q, 0) + s.W - 1, "trace path": s.opening(q, 0) + s.W + 4 * (s.L - 1),
              "quotient row": s.opening(q, 1) + 1, "quotient path": s.opening(q, 1) + 2 * s.Q + 2}
    assert s.L - r - 1 >= 1 and max(places.values()) < ni
    return {name: _bumped(w, pos) for name, pos in places.items()}


def _changed_air(gpu, shape, c, j):
    """The shape's AIR with value j of column c changed: a different AIR of the same shape."""
    _id, kind, args, _log_n, _log_blowup = shape
    if kind == "mimc":
        rc = cases.mimc_constants(args[0]).copy()
        rc[j] = (int(rc[j]) + 1) % P
        return cases.mimc(gpu, args[0], args[1], constants=rc)
    cols = [np.array(col) for col in cases.per_mix_columns(args)]
    cols[c][j] = (int(cols[c][j]) + 1) % P
    return cases.per_mix(gpu, args, columns=cols)


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
    want = [M.verify(oracle, case.air, case.cfg, p) for p in batch]
    assert want[0] == M.OK, dict(zip(names, want))                                  # a changed word is the model's to judge
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
    assert pr.scratch_bytes()[0] == 0 and pr.scratch_bytes()[1] > 0                  # no proving scratch
    pr.close()
    # a different AIR of the same shape: one value of one column changed -> the constraints, nothing else
    cols = case.air.periodic_columns
    for c, j in sorted({(0, 0), (len(cols) - 1, cols[-1].size - 1)}):
        other = _changed_air(gpu, shape, c, j)
        assert M.verify(oracle, other, case.cfg, mine[0]) == M.CONSTRAINTS == 35
        po = case.prover(gpu, other)
        assert po.verify(np.stack([mine[0], mine[0]])).tolist() == [35, 35], (c, j)
        po.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the outer proof
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outer(gpu, oracle):
    """mimc(2, 3) at log_n 3, 3 queries, 4 PoW bits: the inner prover, its verifier circuit, the oracle's copy of it from the
    exported blob, three inner proofs with different public values and their outer proofs."""
    k, d, log_n, log_blowup = MIMC5
    air = cases.mimc(gpu, k, d)
    pr = gpu.P3Prover(air, log_n, log_blowup, 3, 4)
    tp = [cases.mimc_trace(log_n, k, d, x0) for x0 in (1, 11, P - 2)]
    traces, pvs = np.stack([t for t, _ in tp]), np.stack([v for _, v in tp])
    inner, st = pr.prove(traces, public_values=pvs)
    assert st.tolist() == [OK] * 3
    circuit = gpu.Circuit.build_p3_verifier_air(pr.config, air)
    assert int(circuit.info.num_public_inputs) == 2 and int(circuit.info.num_inputs) == pr.num_inputs
    oc = oracle.load_circuit(circuit.to_blob())
    proofs, st = circuit.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [OK] * 3
    yield pr, circuit, oc, traces, pvs, inner, proofs
    pr.close()


def test_outer_proofs_equal_the_oracles(gpu, outer):
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    dg, cap = circuit.digest()
    for i in range(3):
        po, sto, _tm, msg = oc.prove(inner[i], seed=i + 1)
        assert sto == 0, msg
        assert np.array_equal(proofs[i], po), f"outer proof {i} differs from the oracle's"
        assert proofs[i][-2:].tolist() == pvs[i].tolist()
        assert oc.verify(proofs[i], dg, cap)[0] == 0
    assert circuit.verify(proofs).tolist() == [OK] * 3


@pytest.mark.parametrize("j", [0, 3])
def test_a_changed_round_constant_is_a_witness_conflict(gpu, outer, j):
    pr, circuit, oc, traces, pvs, inner, proofs = outer
    k, d, log_n, log_blowup = MIMC5
    rc = cases.mimc_constants(k).copy()
    rc[j] = (int(rc[j]) + 1) % P
    other = gpu.Circuit.build_p3_verifier_air(pr.config, cases.mimc(gpu, k, d, constants=rc))
    assert other.digest()[0].tolist() != circuit.digest()[0].tolist()
    got, st = other.prove(inner, seeds=[1, 2, 3])
    assert st.tolist() == [WITNESS_CONFLICT] * 3


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
