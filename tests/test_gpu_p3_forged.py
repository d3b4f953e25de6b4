"""GPU: the plonky3 verifiers and the device prover on forged proofs from the model prover (tests/p3_prove_model.py,
tests/p3_forged_cases.py): proofs finished honestly from faulted data, which fail exactly one check.  The expected codes are
the table's, written down from the documented order of checks; every comparison is equality.

1. verdicts: per shape one mixed batch through P3Prover.verify and through verify_dev on guard-banded strided buffers
2. batch edges: a 35-forgery first and last among honest proofs, around the 4-proofs-per-wave and 64-lane boundaries
3. precedence of two failures, on the device
4. the device prover: [honest, faulted trace, honest] gives status [0, 1, 0], a zero row and the MODEL prover's words
5. recursion: the verifier circuit's device witness generator refuses each forged proof between two honest ones"""
import numpy as np
import pytest

import p3_aux_model as M
import p3_forged_cases as FC
import p3_prove_model as PV
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097


@pytest.fixture(scope="module", params=FC.SHAPE_IDS)
def shape(request, gpu, oracle):
    b = FC.build(gpu, oracle, request.param)
    pr = gpu.P3Prover(b.air, b.log_n, b.log_blowup, b.queries, b.pow_bits)
    assert pr.num_inputs == b.words.size and b.cfg.same_as(pr.config)
    yield b, pr
    pr.close()


def _handle(gpu, oracle, name):
    b = FC.build(gpu, oracle, name)
    return b, gpu.P3Prover(b.air, b.log_n, b.log_blowup, b.queries, b.pow_bits)


def _dev_verify(pr, proofs, stride):
    """verify_dev on guard-banded buffers whose stride padding holds sentinels >= p; the statuses, after checking that the
    inputs are unchanged and nothing outside the statuses was written."""
    import torch
    n, ni = proofs.shape[0], pr.num_inputs
    d_in, d_st = Banded(n * stride, before=ODD), Banded32(n, before=ODD)
    data, _pad = strided_rows(n, ni, stride)
    interior = d_in.get()
    interior[data] = proofs.ravel()
    d_in.set(interior)
    torch.cuda.synchronize()
    pr.verify_dev(d_in.ptr, n, stride, d_st.ptr, 0)
    pr.sync()
    d_in.assert_unchanged()
    d_st.assert_bands_intact()
    return d_st.get().astype(np.int32)


# ---- 1. verdicts ------------------------------------------------------------------------------------------------------
def test_verdicts_of_the_mixed_batch(shape):
    b, pr = shape
    batch, want, names = FC.mixed(b.forged, b.words, seed=23)
    assert {0, M.FRI_MERKLE, M.FINAL_POLY, M.CONSTRAINTS} <= set(want)
    got = pr.verify(batch).tolist()
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    got = _dev_verify(pr, batch, pr.num_inputs + 3).tolist()
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]


# ---- 2. batch edges -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def range_handle(gpu, oracle):
    b, pr = _handle(gpu, oracle, "range")
    yield b, pr
    pr.close()


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65])
def test_batch_edges_with_a_forgery_first_and_last(range_handle, n):
    b, pr = range_handle
    forged = next(f for f in b.forged if f.kind == "unbalanced")
    assert forged.code == M.CONSTRAINTS
    for at in sorted({0, n - 1}):
        batch = np.tile(b.words, (n, 1))
        batch[at] = forged.proof
        want = [OK] * n
        want[at] = M.CONSTRAINTS
        assert pr.verify(batch).tolist() == want, (n, at)


# ---- 3. precedence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib", "range"])
def test_precedence_of_two_failures(gpu, oracle, name):
    b, pr = _handle(gpu, oracle, name)
    cases = FC.precedence(b)
    want = [c for _p, c in cases.values()]
    assert want == [M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY, M.MALFORMED, M.FRI_MERKLE, M.FINAL_POLY]
    batch = np.stack([p for p, _c in cases.values()] + [b.words])
    assert pr.verify(batch).tolist() == want + [OK], list(cases)
    assert _dev_verify(pr, batch, pr.num_inputs + 3).tolist() == want + [OK], list(cases)
    pr.close()


# ---- 4. the device prover -------------------------------------------------------------------------------------------------
def test_the_device_prover_writes_the_models_words_and_refuses_the_faulted_traces(shape):
    b, pr = shape
    faulted = [f for f in b.forged if f.kind in ("row", "unbalanced", "public")]
    assert len(faulted) >= 2
    traces, pvs = [b.trace], [b.pv]
    for f in faulted:
        traces += [f.trace, b.trace]
        pvs += [f.pv, b.pv]
    n = len(traces)
    pv = np.stack(pvs) if b.pv is not None else None
    words, st = pr.prove(np.stack(traces), public_values=pv, pow_starts=np.full(n, b.pow_start, dtype=np.uint64))
    assert st.tolist() == [OK] + [INVALID_ARG, OK] * len(faulted)
    for i in range(n):
        if i % 2:
            assert not words[i].any(), faulted[i // 2].name
        else:
            assert np.array_equal(words[i], b.words), i      # the MODEL prover's words, not through the host prover
    # and the checker names, on the device, what each fault broke
    reports = pr.check(np.stack(traces), public_values=pv)
    assert [r.first for r in reports] == [None] + [x for f in faulted for x in (f.first, None)]


# ---- 5. recursion -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=FC.RECURSION_IDS)
def outer(request, gpu, oracle):
    """The verifier circuit of the shape, built once, and the oracle's copy of it."""
    b = FC.build(gpu, oracle, request.param)
    cfg = gpu.P3Config(*[getattr(b.cfg, f) for f in PV.Config.FIELDS])
    circuit = gpu.Circuit.build_p3_verifier_air(cfg, b.air)
    assert int(circuit.info.num_inputs) == b.words.size
    return b, circuit, oracle.load_circuit(circuit.to_blob())


def test_the_verifier_circuit_refuses_each_forged_proof_between_two_honest_ones(outer):
    b, circuit, oc = outer
    inner = np.stack([w for f in b.forged for w in (b.words, f.proof, b.words)])
    proofs, st = circuit.prove(inner, seeds=[1] * len(inner))
    assert st.tolist() == [OK, WITNESS_CONFLICT, OK] * len(b.forged), \
        [(f.name, st[3 * i:3 * i + 3].tolist()) for i, f in enumerate(b.forged) if st[3 * i:3 * i + 3].tolist() != [0, 4, 0]]
    assert proofs[0].any()
    for i in range(len(b.forged)):
        assert np.array_equal(proofs[3 * i], proofs[0]) and np.array_equal(proofs[3 * i + 2], proofs[0]), b.forged[i].name
    dg, cap = circuit.digest()
    assert oc.verify(proofs[0], dg, cap)[0] == 0
