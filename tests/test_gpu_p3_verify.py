"""GPU: p25_p3_verify_batch[_dev] (include/p25.h) -- src/p3/verifier.rs run natively on flat plonky3 proofs -- against
the plain-Python model of that verifier (tests/p3_verify_model.py, pinned to the oracle's witness of the reference's
verifier circuit by tests/test_p3_verify_model_cpu.py).  Field arithmetic is exact: every status must EQUAL the model's.

1. accepts: the artifact, device-prover outputs from 2 to 8192 rows, every chunk count, wide and narrow traces
2. all 240 single-word flips of one proof in one batch, and the batch reversed
3. batch sizes around the 4-proofs-per-wave and 64-lane boundaries, the tampered proof first and last
4. precedence of two failures in one proof
5. the six codes by name
6. the device form: strides and guard bands, a caller's stream, chained behind the device prover without a host
   synchronisation, a rejected trace's zero row, no proving scratch, chunks"""
import ctypes as C

import numpy as np
import pytest

import air_cases
import p3_verify_cases as pc
import p3_verify_model as M
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG = 0, 1
ODD = 4097


@pytest.fixture(scope="module")
def fib(gpu):
    """The fib (3, 3, 4) proof, a handle for it and one for the wrong AIR of the same shape."""
    case = pc.flip_case(gpu, pc.FIB334)
    pr, wrong = case.prover(gpu), case.prover(gpu, pc.wrong_air(gpu))
    assert pr.num_inputs == wrong.num_inputs == case.words.size == 240
    yield case, pr, wrong
    pr.close()
    wrong.close()


@pytest.fixture(scope="module")
def flips(gpu, oracle, fib):
    """The untouched proof and its 240 single-word flips, with the model's verdicts (computed once, never changed)."""
    case, _pr, _wrong = fib
    proofs = np.stack([case.words] + [w for _pos, w in pc.all_flips(case.words)])
    want = np.array([M.verify(oracle, case.air, case.cfg, w) for w in proofs], dtype=np.int32)
    assert proofs.shape == (241, 240) and want[0] == M.OK and M.OK not in want[1:]
    proofs.setflags(write=False)
    want.setflags(write=False)
    return proofs, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. accepts
# ---------------------------------------------------------------------------------------------------------------------
def test_accepts_the_references_artifact(gpu, oracle, fib_inputs):
    air = gpu.Air.fibonacci()
    assert M.verify(oracle, air, gpu.P3Config.fib64(), fib_inputs) == M.OK
    pr = gpu.P3Prover(air, 6, 1, 100, 16)
    assert pr.verify(fib_inputs).tolist() == [OK]
    bad = pc.flipped(fib_inputs, 15750)      # the last word: the last digest of the last query's quotient path
    assert pr.verify(np.stack([bad, fib_inputs])).tolist() == [M.verify(oracle, air, gpu.P3Config.fib64(), bad), OK]
    assert pr.scratch_bytes()[0] == 0
    pr.close()


def _device_proof_is_accepted(gpu, oracle, air, trace, log_n, log_blowup, queries, pow_bits):
    """The device prover's proof of `trace`: accepted by the model and by the device; with the last path's last word
    flipped, the model's code."""
    pr = gpu.P3Prover(air, log_n, log_blowup, queries, pow_bits)
    words, st = pr.prove(trace[None])
    assert st.tolist() == [OK]
    cfg = pr.config
    assert M.verify(oracle, air, cfg, words[0]) == M.OK
    bad = pc.flipped(words[0], pr.num_inputs - 1)
    want_bad = M.verify(oracle, air, cfg, bad)
    assert want_bad == M.INPUT_MERKLE
    assert pr.verify(np.stack([words[0], bad, words[0]])).tolist() == [OK, want_bad, OK]
    pr.close()


# degenerate trees (log_n 1, 2), the FRI-tail and tree-form boundaries of the device prover (10, 11), deep paths and many
# queries (13 with 100 queries: 1,500 + 100 x 91 path steps per proof)
@pytest.mark.parametrize("log_n,queries,pow_bits", [(1, 1, 0), (2, 4, 8), (3, 4, 8), (6, 100, 16), (10, 4, 8), (11, 4, 8),
                                                    (13, 100, 16)])
def test_accepts_device_proofs_fibonacci(gpu, oracle, log_n, queries, pow_bits):
    _device_proof_is_accepted(gpu, oracle, gpu.Air.fibonacci(), air_cases.fib_trace(log_n), log_n, 1, queries, pow_bits)


# widths 1 and 64; 1 / 2 / 4 / 8 quotient chunks; log_blowup 4
@pytest.mark.parametrize("name,log_blowup,chunks", [("random_recurrence:1", 1, 1), ("random_recurrence:64", 1, 1), ("cubic", 1, 2),
                                                    ("quartic_map:6", 2, 4), ("sextic", 3, 8), ("fib", 4, 1)])
def test_accepts_device_proofs_of_other_airs(gpu, oracle, name, log_blowup, chunks):
    air, trace = pc.air_and_trace(gpu, name, 4)
    pr = gpu.P3Prover(air, 4, log_blowup, 3, 4)
    assert 1 << pr.config.log_quotient_degree == chunks
    pr.close()
    _device_proof_is_accepted(gpu, oracle, air, trace, 4, log_blowup, 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# 2. every single-word flip in one batch
# ---------------------------------------------------------------------------------------------------------------------
def test_all_flips_in_one_batch_and_reversed(gpu, fib, flips):
    _case, pr, _wrong = fib
    proofs, want = flips
    got = pr.verify(proofs)
    assert np.array_equal(got, want), [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    assert np.array_equal(pr.verify(proofs[::-1].copy()), want[::-1])
    assert set(want.tolist()) == {M.OK, M.POW, M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY}


# ---------------------------------------------------------------------------------------------------------------------
# 3. batch edges: four proofs per wave in the transcript, 64 lanes per wave elsewhere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65])
def test_batch_edges(gpu, fib, flips, n):
    case, pr, _wrong = fib
    proofs, want = flips
    tampered, code = proofs[1 + case.shape.step(2, 1)], int(want[1 + case.shape.step(2, 1)])    # a FRI sibling value
    assert code == M.FRI_MERKLE
    for at in (0, n - 1):
        batch = np.tile(case.words, (n, 1))
        batch[at] = tampered
        expect = [OK] * n
        expect[at] = code
        assert pr.verify(batch).tolist() == expect, (n, at)


# ---------------------------------------------------------------------------------------------------------------------
# 4. precedence, 5. the six codes
# ---------------------------------------------------------------------------------------------------------------------
def _run_named(gpu, oracle, fib, cases):
    case, pr, wrong = fib
    for name, (air, proof, code) in cases.items():
        assert M.verify(oracle, air, case.cfg, proof) == code, name
        handle = pr if air is case.air else wrong
        assert handle.verify(np.stack([case.words, proof])).tolist() == [OK if handle is pr else M.CONSTRAINTS, code], name


def test_precedence_of_double_tampers(gpu, oracle, fib):
    cases = pc.double_tampers(gpu, fib[0])
    assert [c for _a, _p, c in cases.values()] == [M.INPUT_MERKLE, M.FINAL_POLY, M.FRI_MERKLE, M.MALFORMED, M.MALFORMED, M.FINAL_POLY]
    _run_named(gpu, oracle, fib, cases)


def test_the_six_codes(gpu, oracle, fib):
    cases = pc.code_cases(gpu, oracle, fib[0])
    assert {c for _a, _p, c in cases.values()} == {30, 31, 32, 33, 34, 35}
    _run_named(gpu, oracle, fib, cases)


def test_words_at_or_above_p_anywhere(gpu, fib):
    case, pr, _wrong = fib
    s = case.shape
    batch = [case.words]
    for pos in (2, s.o_chunks + 1, s.step(1, 2) + 3, s.o_pow_witness, s.num_inputs - 1):
        for word in (P, (1 << 64) - 1, P + 5):
            batch += [pc.with_word(case.words, pos, word), case.words]
    assert pr.verify(np.stack(batch)).tolist() == [OK] + [M.MALFORMED, OK] * 15


# ---------------------------------------------------------------------------------------------------------------------
# 6. the device form
# ---------------------------------------------------------------------------------------------------------------------
def _dev_verify(pr, proofs, stride, stream=None, occupy=None):
    """verify_dev on guard-banded buffers; returns the statuses after checking that nothing else was written."""
    import torch
    n, ni = proofs.shape[0], pr.num_inputs
    d_in, d_st = Banded(n * stride, before=ODD), Banded32(n, before=ODD)
    data, _pad = strided_rows(n, ni, stride)
    interior = d_in.get()                    # the padding behind a proof keeps its sentinels: words >= p
    interior[data] = proofs.ravel()
    if stream is None:
        d_in.set(interior)
        torch.cuda.synchronize()
    else:
        d_in.set_async(interior, stream, before_enqueue=occupy)
    pr.verify_dev(d_in.ptr, n, stride, d_st.ptr, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    else:
        pr.sync()
    d_in.assert_unchanged()
    d_st.assert_bands_intact()
    return d_st.get().astype(np.int32)


def test_strides_and_guard_bands(gpu, fib, flips):
    _case, pr, _wrong = fib
    proofs, want = flips
    pick = [0, 3, 40, 100, 0, 170, 239, 240, 0]
    for stride in (pr.num_inputs + 3, pr.num_inputs):
        assert np.array_equal(_dev_verify(pr, proofs[pick], stride), want[pick]), stride
    # the host form with a stride: the words behind a proof are not read (here they are >= p)
    rows = np.full((len(pick), pr.num_inputs + 5), P + 9, dtype=np.uint64)
    rows[:, :pr.num_inputs] = proofs[pick]
    keep = rows.copy()
    assert np.array_equal(pr.verify(rows), want[pick]) and np.array_equal(rows, keep)


def test_runs_on_the_callers_stream(gpu, fib, flips):
    """The proofs arrive ON the side stream, as a copy queued behind milliseconds of other work; until the stream gets
    there the buffer holds sentinels (words >= p): a launch anywhere else starts at once and reports MALFORMED."""
    import torch
    _case, pr, _wrong = fib
    proofs, want = flips
    dev = torch.device("cuda", 0)
    lib = gpu.lib()
    n, w = 1 << 19, 135
    cols = torch.randint(0, 1 << 62, (w * n,), dtype=torch.int64, device=dev)
    tree = torch.zeros(int(lib.p25_merkle_tree_words(n, 4)), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    assert pr.verify(proofs[:70]).tolist() == want[:70].tolist()      # tables and scratch exist before the order matters
    torch.cuda.synchronize()

    def occupy():
        assert lib.p25_merkle_commit_dev(C.c_void_p(cols.data_ptr()), n, n, w, 4, C.c_void_p(tree.data_ptr()),
                                         C.c_void_p(side.cuda_stream)) == 0

    got = _dev_verify(pr, proofs[:70], pr.num_inputs + 1, stream=side, occupy=occupy)
    assert np.array_equal(got, want[:70])
    torch.cuda.synchronize()


def test_chained_behind_the_device_prover_with_a_rejected_trace(gpu, oracle, fib):
    """p25_p3_prove_batch_dev -> p25_p3_verify_batch_dev on one stream, no host synchronisation in between: every proof
    is accepted, and the zero row the prover leaves for a trace that violates the AIR gets the model's code for 240
    zeros."""
    import torch
    case, _pr, _wrong = fib
    dev = torch.device("cuda", 0)
    pr = case.prover(gpu)
    n, ni, tw = 6, pr.num_inputs, case.trace.size
    traces = np.tile(case.trace, (n, 1, 1))
    traces[4] = air_cases.bump(case.trace, 5, 2)
    zero_code = M.verify(oracle, case.air, case.cfg, np.zeros(ni, dtype=np.uint64))
    assert zero_code != M.OK
    side = torch.cuda.Stream(device=dev)
    d_tr = torch.from_numpy(traces.view(np.int64).reshape(-1)).to(dev)
    d_ps = torch.from_numpy(np.arange(n, dtype=np.int64) * 1000).to(dev)
    d_in = torch.full((n * ni,), -1, dtype=torch.int64, device=dev)
    d_pst = torch.full((n,), 77, dtype=torch.int32, device=dev)
    d_vst = torch.full((n,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.data_ptr(), tw, n, d_ps.data_ptr(), d_in.data_ptr(), ni, d_pst.data_ptr(), side.cuda_stream)
    pr.verify_dev(d_in.data_ptr(), n, ni, d_vst.data_ptr(), side.cuda_stream)
    pr.sync()                                       # p25_p3_prover_sync waits for the verifying call too
    assert d_pst.cpu().tolist() == [OK, OK, OK, OK, INVALID_ARG, OK]
    assert d_vst.cpu().tolist() == [OK, OK, OK, OK, zero_code, OK]
    words = d_in.cpu().numpy().view(np.uint64).reshape(n, ni)
    assert not words[4].any() and len({w.tobytes() for w in words}) == n     # distinct PoW witnesses, distinct proofs
    for w in words[:2]:
        assert M.verify(oracle, case.air, case.cfg, w) == M.OK
    assert pr.scratch_bytes()[0] > 0
    pr.close()


def test_a_handle_that_only_verifies_takes_no_proving_scratch(gpu, fib, flips):
    import torch
    case, _pr, _wrong = fib
    proofs, want = flips
    pr = case.prover(gpu)
    assert pr.scratch_bytes() == (0, 0)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    assert np.array_equal(pr.verify(proofs), want)
    proving, verifying = pr.scratch_bytes()
    # 8 + 2 log_n + queries + 2 queries log_n words per proof (include/p25.h)
    assert proving == 0 and verifying == 241 * (8 + 6 + 3 + 18) * 8
    assert free_before - torch.cuda.mem_get_info(0)[0] <= 64 << 20
    pr.close()


def test_chunks_change_no_verdict(gpu, fib, flips):
    case, _pr, _wrong = fib
    proofs, want = flips
    pr = case.prover(gpu)
    per_proof = (8 + 6 + 3 + 18) * 8
    for budget, chunk in ((1, 1), (5 * per_proof, 5), (64 * per_proof + 8, 64)):
        pr.set_scratch_budget(budget)
        assert np.array_equal(pr.verify(proofs), want), budget
    assert pr.scratch_bytes() == (0, 64 * per_proof)         # grown to the largest chunk, never to the batch
    pr.set_scratch_budget(0)
    assert np.array_equal(pr.verify(proofs[::-1].copy()), want[::-1])
    assert pr.scratch_bytes() == (0, 241 * per_proof)
    pr.close()
