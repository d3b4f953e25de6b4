"""GPU: WHERE the entry points read and write in their caller's memory -- strides, streams, guard bands.

The rest of the suite pins the prover to the oracle on values; bench.py, plonky25_amd.aggregate, the C clients and every
tool under tools/ use the device-resident surface (the *_dev entry points, strides, caller streams), which this module
pins: every buffer handed over is the interior of a guard-banded allocation (tests/device_buffers.py) filled with
sentinels in [p, 2^64), every case compares with the oracle -- or with the host entry point on inputs where the suite
already pins that one to the oracle -- and every case ends with the bands of every buffer it handed over, inputs
included, intact.  No case can leave its allocation: every shape is one the library accepts, sized as include/p25.h says,
and the one refusal probed below stays inside its buffer even where the check is missing.

GPU AddressSanitizer is not an option on shared machines; guard bands inside one allocation are the tool there is."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, P, splitmix_field
from device_buffers import Banded, Banded32, banded_host, strided_rows

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, WITNESS_CONFLICT = 0, 1, 4
ODD = 4097            # a band of an odd number of words: the interior is 8-byte aligned and no more


def _sync():
    import torch
    torch.cuda.synchronize()


def _ok(lib, status):
    assert status == OK, lib.p25_last_error().decode()


def _stream_ptr(stream):
    return C.c_void_p(stream.cuda_stream if stream is not None else None)


# ---------------------------------------------------------------------------------------------------------------------
# the three device primitives: one runner each, shared by the plain cases and the caller-stream cases
# ---------------------------------------------------------------------------------------------------------------------
def _feed(buf, data, stream, occupy):
    """The input: a blocking copy, or -- caller-stream cases -- `occupy()` puts its long predecessor on the stream and
    the input follows it there as a non-blocking copy from pinned memory.  Every other buffer of the case exists by
    now, so nothing but the entry point's own call stands between this and the launch."""
    if stream is None:
        buf.set(data)
    else:
        buf.set_async(data, stream, before_enqueue=occupy)


def _run_permute_dev(gpu, oracle, n, seed, stream=None, occupy=None, before=ODD):
    lib = gpu.lib()
    states = splitmix_field(12 * n, seed=seed).reshape(n, 12)
    if n >= 2:
        states[0, :] = P - 1
        states[1, :] = 0
    buf = Banded(12 * n, before=before)
    _feed(buf, states, stream, occupy)
    _ok(lib, lib.p25_poseidon_permute_dev(C.c_void_p(buf.ptr), n, _stream_ptr(stream)))
    stream.synchronize() if stream is not None else _sync()
    got = buf.get().reshape(n, 12)
    assert (got == oracle.poseidon_permute(states)).all() if n else got.size == 0
    buf.assert_bands_intact()            # the words behind 12 * n, and the ones in front


def _run_merkle_dev(gpu, oracle, n, w, cap, stride, seed, stream=None, occupy=None, before=ODD):
    lib = gpu.lib()
    leaves = splitmix_field(n * w, seed=seed).reshape(n, w)                 # row-major, the oracle's layout
    words = (w - 1) * stride + n                                            # what include/p25.h says is read, no more
    cols = Banded(words, before=before)
    data, pad = strided_rows(w, n, stride)
    pad = pad[pad < words]
    interior = cols.expect[cols.before:cols.before + words].copy()          # sentinels stay in the padding
    interior[data] = np.ascontiguousarray(leaves.T).ravel()
    tw = int(lib.p25_merkle_tree_words(n, cap))
    assert tw > 0
    tree = Banded(tw, before=before + 2)
    _feed(cols, interior, stream, occupy)
    _ok(lib, lib.p25_merkle_commit_dev(C.c_void_p(cols.ptr), stride, n, w, cap, C.c_void_p(tree.ptr), _stream_ptr(stream)))
    stream.synchronize() if stream is not None else _sync()
    cap_o, tree_o = oracle.merkle_commit(leaves, cap, want_tree=True)
    got = tree.get()
    diff = np.nonzero(got != tree_o)[0]
    assert diff.size == 0, f"tree words {diff[:8].tolist()} of {tw} differ (n={n} w={w} cap={cap} stride={stride})"
    assert (got[tw - (4 << cap):].reshape(-1, 4) == cap_o).all()            # the cap is the tree's last 4 << cap words
    tree.assert_bands_intact()
    cols.assert_untouched(pad)
    cols.assert_unchanged()


def _run_lde_dev(gpu, oracle, log_n, rate, from_coeffs, with_tree, n_polys, seed, stream=None, occupy=None, before=ODD):
    lib = gpu.lib()
    n, big = 1 << log_n, 1 << (log_n + rate)
    cap = min(4, log_n + rate)
    vals = splitmix_field(n * n_polys, seed=seed).reshape(n_polys, n)
    polys = Banded(n * n_polys, before=before)
    coeffs = None if from_coeffs else Banded(n * n_polys, before=before + 1)   # exactly n_polys << log_n words each
    tmp = None if from_coeffs else Banded(n * n_polys, before=before + 3)
    lde = Banded(big * n_polys, before=before + 5)
    tw = int(lib.p25_merkle_tree_words(big, cap))
    tree = Banded(tw, before=before + 7) if with_tree else None
    ptr = lambda b: C.c_void_p(b.ptr) if b is not None else None              # noqa: E731
    _feed(polys, vals, stream, occupy)
    _ok(lib, lib.p25_lde_commit_dev(ptr(polys), log_n, n_polys, int(from_coeffs), rate, cap, ptr(coeffs), ptr(tmp),
                                    ptr(lde), ptr(tree), _stream_ptr(stream)))
    stream.synchronize() if stream is not None else _sync()
    co, lo, capo = oracle.lde_commit(vals, rate, cap, from_coeffs)
    what = (log_n, rate, from_coeffs, with_tree)
    if from_coeffs:
        assert (co == vals).all()                                              # the input words are the coefficients
    else:
        assert (coeffs.get().reshape(n_polys, n) == co).all(), what
    assert (lde.get().reshape(n_polys, big) == lo).all(), what
    if with_tree:
        t = tree.get()
        assert (t[tw - (4 << cap):].reshape(-1, 4) == capo).all(), what
        _c, tree_o = oracle.merkle_commit(np.ascontiguousarray(lo.T), cap, want_tree=True)
        assert (t == tree_o).all(), what
    polys.assert_unchanged()                                                   # bit-identical afterwards, bands included
    for b in (coeffs, tmp, lde, tree):
        if b is not None:
            b.assert_bands_intact()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 5000])
def test_poseidon_permute_dev(gpu, oracle, n):
    _run_permute_dev(gpu, oracle, n, seed=400 + n, before=ODD if n & 1 else 4096)


MERKLE_SHAPES = [(16, 3, 4), (64, 4, 2), (256, 5, 0), (1024, 8, 4), (2048, 9, 4), (512, 135, 4), (4096, 20, 4),
                 (32, 16, 5), (16, 1, 0),              # the shapes of test_gpu_primitives.test_merkle_vs_oracle
                 (8, 4, 3), (128, 3, 7),               # cap_height == log2(n_leaves): no level kernel runs
                 (128, 4, 0), (2, 1, 0)]               # cap_height 0, down to the smallest tree with a level


@pytest.mark.parametrize("n,w,cap", MERKLE_SHAPES)
def test_merkle_commit_dev_with_column_stride(gpu, oracle, n, w, cap):
    """A leaf of at most four words is its own digest, so with widths 1, 3 and 4 a mis-strided read lands in the tree
    verbatim -- and what it lands on is a sentinel, since the padding between the columns holds them."""
    for k, stride in enumerate((n, n + 1, n + 37, 2 * n)):
        _run_merkle_dev(gpu, oracle, n, w, cap, stride, seed=n * 131 + w + k, before=ODD if k & 1 else 4096)


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("log_n", [3, 10, 11, 13, 16])
def test_lde_commit_dev(gpu, oracle, log_n, rate, from_coeffs):
    """With and without d_tree; with from_coeffs, d_coeffs and d_tmp are NULL."""
    for with_tree in (True, False):
        _run_lde_dev(gpu, oracle, log_n, rate, from_coeffs, with_tree, n_polys=3, seed=900 + 7 * log_n + rate,
                     before=ODD if with_tree else 4096)


# ---------------------------------------------------------------------------------------------------------------------
# caller stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def busy_stream(gpu):
    """A torch side stream and a way to keep it busy: a 2^19-leaf, 135-column Merkle commit through the same entry point
    (the largest launch of a proof, several milliseconds), enqueued on that stream."""
    import torch
    dev = torch.device("cuda", 0)
    n, w = 1 << 19, 135
    cols = torch.randint(0, 1 << 62, (w * n,), dtype=torch.int64, device=dev)       # canonical words (< p)
    tree = torch.zeros(int(gpu.lib().p25_merkle_tree_words(n, 4)), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def occupy():
        lib = gpu.lib()
        _ok(lib, lib.p25_merkle_commit_dev(C.c_void_p(cols.data_ptr()), n, n, w, 4, C.c_void_p(tree.data_ptr()),
                                           C.c_void_p(side.cuda_stream)))

    yield side, occupy
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["poseidon_permute_dev", "merkle_commit_dev", "lde_commit_dev/values",
                                   "lde_commit_dev/coeffs"])
def test_entry_point_runs_on_the_callers_stream(gpu, oracle, busy_stream, which):
    """Every launch goes to the stream the caller names.  Why a launch anywhere else would race here: the side stream
    is a torch pool stream, created non-blocking, so neither the NULL stream nor any other stream waits for it.  It is
    first given milliseconds of work (the 135-column Merkle commit); the entry point's input is then produced ON that
    stream, as a non-blocking copy from pinned host memory queued behind that work, and until the stream gets there the
    input buffer holds sentinels.  A kernel launched on another stream starts at once, reads sentinels -- words >= p,
    never what the oracle was given -- and its result is wrong; a later kernel of the entry point launched elsewhere
    (a tree level, the LDE after the inverse transform) reads what its predecessor has not written yet.  The result is
    read after stream.synchronize() only: nothing else orders the host behind the work."""
    side, occupy = busy_stream
    if which == "poseidon_permute_dev":
        _run_permute_dev(gpu, oracle, 5000, seed=31, stream=side, occupy=occupy)
    elif which == "merkle_commit_dev":
        _run_merkle_dev(gpu, oracle, 4096, 20, 4, 4096 + 37, seed=32, stream=side, occupy=occupy)
    else:
        _run_lde_dev(gpu, oracle, 13, 3, which.endswith("coeffs"), True, n_polys=3, seed=33, stream=side, occupy=occupy)


# ---------------------------------------------------------------------------------------------------------------------
# the refusal p25_lde_commit_dev lacked
# ---------------------------------------------------------------------------------------------------------------------
def test_lde_commit_dev_refuses_a_cap_above_the_leaves(gpu):
    """cap_height > log_n + rate_bits with d_tree: p25_merkle_tree_words answers 0 for that shape and the host form
    refuses it; the device form launched the leaf kernel, which writes 4 << (log_n + rate_bits) words into d_tree.
    log_n 2, rate_bits 1, cap_height 4: d_tree is given 4 << 3 words here, so even a library without the check stays
    inside the allocation -- this probes a missing check, it is not a fault test.  INVALID_ARG, and no word of any
    buffer changed."""
    lib = gpu.lib()
    log_n, rate, cap, n_polys = 2, 1, 4, 2
    assert lib.p25_merkle_tree_words(1 << (log_n + rate), cap) == 0
    polys = Banded(n_polys << log_n)
    polys.set(splitmix_field(n_polys << log_n, seed=5))
    coeffs, tmp = Banded(n_polys << log_n, before=ODD), Banded(n_polys << log_n)
    lde, tree = Banded(n_polys << (log_n + rate)), Banded(4 << (log_n + rate), before=ODD)
    for from_coeffs in (0, 1):
        st = lib.p25_lde_commit_dev(C.c_void_p(polys.ptr), log_n, n_polys, from_coeffs, rate, cap, C.c_void_p(coeffs.ptr),
                                    C.c_void_p(tmp.ptr), C.c_void_p(lde.ptr), C.c_void_p(tree.ptr), None)
        _sync()
        assert st == INVALID_ARG and "cap_height" in lib.p25_last_error().decode()
        for b in (polys, coeffs, tmp, lde, tree):
            b.assert_unchanged()
    # the same shape without d_tree is refused too (the host form's rule, whatever the outputs asked for)
    st = lib.p25_lde_commit_dev(C.c_void_p(polys.ptr), log_n, n_polys, 0, rate, cap, C.c_void_p(coeffs.ptr),
                                C.c_void_p(tmp.ptr), C.c_void_p(lde.ptr), None, None)
    _sync()
    assert st == INVALID_ARG
    for b in (polys, coeffs, tmp, lde):
        b.assert_unchanged()
    # and the largest cap the shape has is accepted: the leaf digests are the cap
    st = lib.p25_lde_commit_dev(C.c_void_p(polys.ptr), log_n, n_polys, 0, rate, log_n + rate, C.c_void_p(coeffs.ptr),
                                C.c_void_p(tmp.ptr), C.c_void_p(lde.ptr), C.c_void_p(tree.ptr), None)
    _sync()
    assert st == OK
    for b in (polys, coeffs, tmp, lde, tree):
        b.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------
# proofs at a stride
# ---------------------------------------------------------------------------------------------------------------------
N_MAX = 65            # one more than a witness pass (64); 17 is one more than the stream pool (16)


class _Batch:
    """One circuit with N_MAX distinct inputs, their seeds, and the reference: the proofs p25_prove_batch returns at
    stride == proof_words (the path test_gpu_prover / test_gpu_gadgets pin to the oracle)."""

    def __init__(self, name, circuit, oc, inputs, spoil):
        self.name, self.c, self.oc, self.inputs, self.spoil = name, circuit, oc, inputs, spoil
        self.pw, self.ni = int(circuit.info.proof_words), int(circuit.info.num_inputs)
        assert inputs.shape == (N_MAX, self.ni)
        self.seeds = np.arange(N_MAX, dtype=np.uint64) + np.uint64(100)
        self._ref, self._oracle = {}, {}

    def batch(self, n):
        """(inputs, seeds, expected statuses) of the first n proofs, the middle one (n >= 3) with a wrong expectation."""
        inp, want = self.inputs[:n].copy(), np.zeros(n, dtype=np.int64)
        if n >= 3:
            inp[n // 2] = self.spoil(inp[n // 2])
            want[n // 2] = WITNESS_CONFLICT
        return inp, self.seeds[:n].copy(), want

    def reference(self, n):
        if n not in self._ref:
            inp, seeds, want = self.batch(n)
            proofs, st = self.c.prove(inp, seeds=seeds)
            assert st.tolist() == want.tolist(), (self.name, n, st.tolist())
            self._ref[n] = proofs
        return self._ref[n]

    def oracle_proof(self, i):
        if i not in self._oracle:
            po, sto, _tm, msg = self.oc.prove(self.inputs[i], seed=int(self.seeds[i]))
            assert sto == 0, msg
            self._oracle[i] = po
        return self._oracle[i]

    def check(self, n, got, status, want):
        """got[n][pw]: every good proof equals the host entry point's, proofs 0 / 16 / 64 equal the oracle's."""
        assert status.tolist() == want.tolist(), (self.name, n, status.tolist())
        ref = self.reference(n)
        for i in range(n):
            if want[i] == 0:
                diff = np.nonzero(got[i] != ref[i])[0]
                assert diff.size == 0, f"{self.name}: proof {i} of {n}: first differing words {diff[:8].tolist()}"
        for i in (0, 16, 64):
            if i < n and want[i] == 0:
                assert (got[i] == self.oracle_proof(i)).all(), (self.name, n, i)


@pytest.fixture(scope="module")
def batches(gpu, oracle):
    out = {}
    # the `and` gadget: different operands per proof
    c = gpu.Circuit.build_gadget(0, 0)
    xs, ys = splitmix_field(N_MAX, seed=61), splitmix_field(N_MAX, seed=62)
    inp = np.stack([xs, ys, (xs & ys) % np.uint64(P)], axis=1)

    def spoil_and(row):
        row = row.copy()
        row[2] = (int(row[2]) + 1) % P
        return row

    out["and"] = _Batch("and", c, oracle.load_circuit(c.to_blob()), inp, spoil_and)
    # the 2^10-row plonky3 verifier of stage_circuits.build_small: proofs of the same STARK with different PoW
    # witnesses (different query indices), where the grind finds different ones
    base, cfg = gpu.p3_prove_fibonacci(3, 3, 4)
    rows = []
    for k in range(N_MAX):
        v, cfg_k = gpu.p3_prove_fibonacci(3, 3, 4, pow_start=1000 * k)
        assert bytes(cfg_k) == bytes(cfg) and v.shape == base.shape
        rows.append(v)
    inp = np.stack(rows)
    assert len({r.tobytes() for r in rows}) > N_MAX // 2, "the PoW variants are not distinct"
    c = gpu.Circuit.build_p3_verifier(cfg)
    assert int(c.info.degree_bits) == 10
    oc = oracle.load_circuit(c.to_blob())

    def spoil_p3(row):
        row = row.copy()
        row[0] = (int(row[0]) + 1) % P
        return row

    assert oc.witness(spoil_p3(inp[1]), seed=0)[1] == WITNESS_CONFLICT       # the checker agrees that this is a bad proof
    out["p3_small"] = _Batch("p3_small", c, oc, inp, spoil_p3)
    yield out
    for b in out.values():
        b.c.close()


def _rows(interior, n, stride, pw):
    return interior.reshape(n, stride)[:, :pw] if n else interior.reshape(0, pw)


@pytest.mark.parametrize("extra", [0, 1, 13])
@pytest.mark.parametrize("n", [0, 1, 3, 17, 65])
@pytest.mark.parametrize("name", ["and", "p3_small"])
def test_prove_batch_dev_at_a_stride(gpu, batches, name, n, extra):
    b = batches[name]
    stride = b.pw + extra
    inp, seeds, want = b.batch(n)
    d_in, d_seeds = Banded(n * b.ni, before=ODD), Banded(n)
    d_in.set(inp)
    d_seeds.set(seeds)
    d_proofs, d_status = Banded(n * stride, before=ODD if extra & 1 else 4096), Banded32(n, before=ODD)
    lib = gpu.lib()
    _ok(lib, lib.p25_prove_batch_dev(b.c._h, C.c_void_p(d_in.ptr), n, C.c_void_p(d_seeds.ptr), C.c_void_p(d_proofs.ptr),
                                     stride, C.c_void_p(d_status.ptr), None))
    b.c.sync()
    _sync()
    _data, pad = strided_rows(n, b.pw, stride)
    d_proofs.assert_untouched(pad)                     # every padding word, the failing proof's included
    d_proofs.assert_bands_intact()
    d_status.assert_bands_intact()                     # the status words behind n_proofs
    d_in.assert_unchanged()
    d_seeds.assert_unchanged()
    if n == 0:
        return                                         # P25_OK and nothing written: the bands are all there is
    b.check(n, _rows(d_proofs.get(), n, stride, b.pw), d_status.get().astype(np.int64), want)


@pytest.mark.parametrize("name", ["and", "p3_small"])
def test_prove_batch_dev_refuses_a_stride_below_the_proof(gpu, batches, name):
    b = batches[name]
    inp, seeds, _want = b.batch(1)
    d_in, d_seeds, d_proofs, d_status = Banded(b.ni), Banded(1), Banded(b.pw), Banded32(1)
    d_in.set(inp)
    d_seeds.set(seeds)
    lib = gpu.lib()
    st = lib.p25_prove_batch_dev(b.c._h, C.c_void_p(d_in.ptr), 1, C.c_void_p(d_seeds.ptr), C.c_void_p(d_proofs.ptr),
                                 b.pw - 1, C.c_void_p(d_status.ptr), None)
    b.c.sync()
    _sync()
    assert st == INVALID_ARG
    for buf in (d_in, d_seeds, d_proofs, d_status):
        buf.assert_unchanged()


@pytest.mark.parametrize("name", ["and", "p3_small"])
def test_host_batch_entry_points_at_a_stride(gpu, batches, name):
    """p25_prove_batch and p25_prove_batch_filler with proof_stride_words > proof_words, into numpy guard buffers: the
    same equalities, untouched padding, intact bands.  The filler values are the ones the seeds stand for (read back
    from the oracle's witness, as test_gpu_prover does), so the filler path must give the very same proofs."""
    b = batches[name]
    n, extra = 5, 13
    stride = b.pw + extra
    inp, seeds, want = b.batch(n)
    lib = gpu.lib()
    _data, pad = strided_rows(n, b.pw, stride)
    inp_c = np.ascontiguousarray(inp)
    # seeds
    out, st = banded_host(n * stride, before=ODD), banded_host(n, dtype=np.uint32)
    _ok(lib, lib.p25_prove_batch(b.c._h, inp_c.ctypes.data_as(C.c_void_p), n, seeds.ctypes.data_as(C.c_void_p), out.ptr, stride,
                                 st.ptr, None))
    out.assert_untouched(pad)
    out.assert_bands_intact()
    st.assert_bands_intact()
    b.check(n, _rows(out.get(), n, stride, b.pw), st.get().astype(np.int64), want)
    # n_proofs == 0: P25_OK, nothing written
    out0, st0 = banded_host(stride), banded_host(1, dtype=np.uint32)
    _ok(lib, lib.p25_prove_batch(b.c._h, inp_c.ctypes.data_as(C.c_void_p), 0, None, out0.ptr, stride, st0.ptr, None))
    out0.assert_unchanged()
    st0.assert_unchanged()
    # the binding's proof_stride: proofs in the first proof_words words of each row, zeros behind them
    via, st_b = b.c.prove(inp, seeds=seeds, proof_stride=stride)
    assert via.shape == (n, stride) and not via[:, b.pw:].any()
    b.check(n, via[:, :b.pw], st_b.astype(np.int64), want)
    # explicit filler
    nf = int(b.c.info.num_random_fill)
    filler = np.zeros((n, nf), dtype=np.uint64)
    for i in range(n):
        wo, _s, _m = b.oc.witness(b.inputs[i], seed=int(seeds[i]))    # the unspoiled input: the filler follows the seed alone
        cand = np.nonzero((wo[:4] == 0).all(axis=0) & (wo[4:] != 0).all(axis=0))[0]
        assert cand.size >= 1 and wo[4:, cand[0]].size == nf
        filler[i] = wo[4:, cand[0]]
    out, st = banded_host(n * stride), banded_host(n, before=ODD, dtype=np.uint32)
    _ok(lib, lib.p25_prove_batch_filler(b.c._h, inp_c.ctypes.data_as(C.c_void_p), n, filler.ctypes.data_as(C.c_void_p),
                                        out.ptr, stride, st.ptr))
    out.assert_untouched(pad)
    out.assert_bands_intact()
    st.assert_bands_intact()
    b.check(n, _rows(out.get(), n, stride, b.pw), st.get().astype(np.int64), want)
    via, st_b = b.c.prove_filler(inp, filler, proof_stride=stride)
    assert via.shape == (n, stride) and not via[:, b.pw:].any()
    b.check(n, via[:, :b.pw], st_b.astype(np.int64), want)


def test_prove_batch_dev_windows_at_an_output_stride(gpu):
    """The three-leaf, 2-ary case of tests/c_abi/chain.c from Python: groups (0, 1) and, right-aligned and overlapping,
    (1, 2), proved in one batch straight on the leaves' buffer, the aggregates written at a stride above the
    aggregator's proof words.  The host path proves the two groups from explicit copies and must give the same words."""
    leaf = gpu.Circuit.build_gadget(0, 0)
    agg = leaf.build_aggregator(2)
    lw, aw = int(leaf.info.proof_words), int(agg.info.proof_words)
    assert int(agg.info.num_inputs) == 2 * lw
    ops = [(0x0123456789ABCDEF, 0x0FEDCBA987654321), (0x1111222233334444, 0x00FF00FF00FF00FF),
           (0x5555AAAA5555AAAA, 0x0F0F0F0FF0F0F0F0)]
    inp = np.array([[x, y, x & y] for x, y in ops], dtype=np.uint64)
    leaves, st = leaf.prove(inp, seeds=[7, 8, 11])
    assert st.tolist() == [0, 0, 0]
    seeds_w = np.array([9, 10], dtype=np.uint64)
    ref, st = agg.prove(np.stack([leaves[0:2].ravel(), leaves[1:3].ravel()]), seeds=seeds_w)
    assert st.tolist() == [0, 0]
    stride = aw + 7
    d_leaves, d_seeds = Banded(3 * lw, before=ODD), Banded(2)
    d_leaves.set(leaves)
    d_seeds.set(seeds_w)
    d_out, d_status = Banded(2 * stride, before=ODD), Banded32(2)
    agg.prove_dev_windows(d_leaves.ptr, 2 * lw, 1 * lw, 2, d_seeds.ptr, d_out.ptr, stride, d_status.ptr)
    agg.sync()
    _sync()
    assert d_status.get().tolist() == [0, 0]
    got = _rows(d_out.get(), 2, stride, aw)
    assert (got == ref).all(), np.argwhere(got != ref)[:5]
    d_out.assert_untouched(strided_rows(2, aw, stride)[1])
    for b in (d_out, d_status):
        b.assert_bands_intact()
    d_leaves.assert_unchanged()
    d_seeds.assert_unchanged()
    agg.close()
    leaf.close()


def test_gather_proofs_moves_whole_strides():
    """p25_gather_proofs in a world of one (tests/_gather_stride_worker.py, a child process as in test_gpu_nccl.py):
    stride = proof words + 5; all n * stride words arrive, padding included, and the destination's bands are intact."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gather_stride_worker.py")], capture_output=True,
                       text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "GATHER_STRIDE_OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# host outputs sized exactly as documented
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(gpu, oracle):
    import stage_circuits
    c, oc, wires = stage_circuits.build_small(gpu, oracle)
    inp, _cfg = gpu.p3_prove_fibonacci(3, 3, 4)
    return c, oc, wires, inp


def _in(a):
    return np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(C.c_void_p)


def _finish(out, want, what):
    got = out.get()
    want = np.ascontiguousarray(want).ravel()
    assert got.size == want.size and (got == want).all(), what
    out.assert_bands_intact()


def test_host_outputs_of_the_stage_entry_points_are_exactly_as_large_as_documented(gpu, oracle, small):
    """p25_witness, p25_partial_products, p25_quotient, p25_circuit_digest on the small circuit: each output in a
    guard-banded numpy buffer of exactly the documented size, compared with the oracle as test_gpu_stages does."""
    c, oc, wires, inp = small
    lib, info = gpu.lib(), c.info
    n, nw = 1 << int(info.degree_bits), int(info.num_wires)
    nc, npp, qdf = int(info.num_challenges), int(info.num_partial_products), int(info.quotient_degree_factor)
    betas, gammas, alphas = splitmix_field(6, seed=11).reshape(3, 2)
    # p25_witness: wires_out[num_wires][2^degree_bits]
    out, st = banded_host(nw * n, before=ODD), C.c_int32(99)
    _ok(lib, lib.p25_witness(c._h, _in(inp), 3, out.ptr, C.byref(st)))
    assert st.value == 0
    _finish(out, wires, "witness")
    # p25_partial_products: out[NC * (1 + NP)][n]
    zo = oc.partial_products(wires, betas, gammas)
    assert zo.shape == (nc * (1 + npp), n)
    out = banded_host(nc * (1 + npp) * n, before=ODD)
    _ok(lib, lib.p25_partial_products(c._h, _in(wires), _in(betas), _in(gammas), out.ptr))
    _finish(out, zo, "partial products")
    # p25_quotient: out[NC * quotient_degree_factor][n]
    qo = oc.quotient(wires, zo, betas, gammas, alphas)
    assert qo.shape == (nc * qdf, n)
    out = banded_host(nc * qdf * n, before=ODD)
    _ok(lib, lib.p25_quotient(c._h, _in(wires), _in(zo), _in(betas), _in(gammas), _in(alphas), out.ptr))
    _finish(out, qo, "quotient")
    # p25_circuit_digest: digest4 and the cap [2^cap_height][4] (cap_height 4 in the standard configuration)
    do, capo = oc.digest()
    dg, cap = banded_host(4, before=ODD), banded_host(capo.size)
    _ok(lib, lib.p25_circuit_digest(c._h, dg.ptr, cap.ptr))
    _finish(dg, do, "digest")
    _finish(cap, capo, "constants/sigmas cap")


def test_host_outputs_of_the_primitive_entry_points_are_exactly_as_large_as_documented(gpu, oracle):
    lib = gpu.lib()
    # p25_eval_polys: out[n_polys][2]
    log_n, n_polys = 10, 7
    coeffs, zeta = splitmix_field(n_polys << log_n, seed=80).reshape(n_polys, 1 << log_n), splitmix_field(2, seed=71)
    out = banded_host(2 * n_polys, before=ODD)
    _ok(lib, lib.p25_eval_polys(_in(coeffs), n_polys, log_n, _in(zeta), 1, out.ptr))
    _finish(out, oracle.eval_polys(coeffs, zeta, 1), "eval_polys")
    # p25_fri_prove: exactly p25_fri_prove_words
    log_n, rate, cap_h, arity, pow_bits, queries = 10, 3, 4, np.array([4, 4], dtype=np.int32), 8, 5
    fc, seed = splitmix_field(2 << log_n, seed=1010).reshape(2, 1 << log_n), splitmix_field(13, seed=99)
    words = int(lib.p25_fri_prove_words(log_n, rate, cap_h, arity.ctypes.data_as(C.c_void_p), 2, queries))
    want = oracle.fri_prove(fc, rate, cap_h, arity, pow_bits, queries, seed)
    assert words == want.size
    out, st = banded_host(words, before=ODD), C.c_int32(99)
    _ok(lib, lib.p25_fri_prove(_in(fc), log_n, rate, cap_h, arity.ctypes.data_as(C.c_void_p), 2, pow_bits, queries, _in(seed),
                               seed.size, out.ptr, words, C.byref(st)))
    assert st.value == 0
    _finish(out, want, "fri_prove")
    # p25_transcript: challenges_out[sum n_challenges]
    segs = [(splitmix_field(9, seed=1), 2), (splitmix_field(0, seed=2), 0), (splitmix_field(17, seed=3), 7),
            (splitmix_field(1, seed=4), 29)]
    obs = np.concatenate([w for w, _ in segs])
    lens, nch = np.array([w.size for w, _ in segs], dtype=np.uint32), np.array([k for _, k in segs], dtype=np.uint32)
    out = banded_host(int(nch.sum()), before=ODD)
    _ok(lib, lib.p25_transcript(_in(obs), lens.ctypes.data_as(C.c_void_p), nch.ctypes.data_as(C.c_void_p), len(segs), out.ptr))
    _finish(out, oracle.transcript(segs), "transcript")
    # p25_merkle_commit with tree_out: cap_out[2^cap][4], tree_out[p25_merkle_tree_words]
    for n, w, cap_h in ((64, 4, 2), (2048, 9, 4), (16, 3, 4)):
        leaves = splitmix_field(n * w, seed=n + w).reshape(n, w)
        cap_o, tree_o = oracle.merkle_commit(leaves, cap_h, want_tree=True)
        cap, tree = banded_host(4 << cap_h, before=ODD), banded_host(int(lib.p25_merkle_tree_words(n, cap_h)))
        _ok(lib, lib.p25_merkle_commit(_in(leaves.T), n, w, cap_h, cap.ptr, tree.ptr))
        _finish(cap, cap_o, "merkle cap")
        _finish(tree, tree_o, "merkle tree")
    # p25_lde_commit: coeffs_out[n_polys][n], lde_out[n_polys][n << rate], cap_out[2^cap][4]
    for log_n, rate, from_coeffs in ((3, 1, False), (11, 3, False), (12, 2, True)):
        n_polys, cap_h = 3, min(4, log_n + rate)
        vals = splitmix_field(n_polys << log_n, seed=log_n).reshape(n_polys, 1 << log_n)
        co, lo, capo = oracle.lde_commit(vals, rate, cap_h, from_coeffs)
        bc, bl, bcap = (banded_host(n_polys << log_n, before=ODD), banded_host(n_polys << (log_n + rate)),
                        banded_host(4 << cap_h, before=ODD))
        _ok(lib, lib.p25_lde_commit(_in(vals), log_n, n_polys, int(from_coeffs), rate, cap_h, bc.ptr, bl.ptr, bcap.ptr))
        _finish(bc, co, "lde coeffs")
        _finish(bl, lo, "lde")
        _finish(bcap, capo, "lde cap")


# ---------------------------------------------------------------------------------------------------------------------
# the LDE over the domain p25_lde_commit accepts: log_n 0..20, rate_bits 0..3
# ---------------------------------------------------------------------------------------------------------------------
def _lde_input(log_n, n_polys, case):
    """Half the cases take edge_values columns, half uniform words."""
    import edge_values as ev
    n = 1 << log_n
    if case & 1:
        return splitmix_field(n * n_polys, seed=3000 + case).reshape(n_polys, n)
    fills = [ev.edge(n, 40 + case), ev.const(n, P - 1), ev.alternating(n, P - 1, 0), ev.high(n, 41 + case),
             ev.delta(n, n - 1, P - 1), ev.mixed(n, 42 + case)]
    return np.stack([fills[(case // 2 + k) % len(fills)] for k in range(n_polys)])


@pytest.mark.parametrize("log_n", list(range(17)))
def test_lde_commit_over_the_accepted_domain(gpu, oracle, log_n):
    """p25_lde_commit == oracle.lde_commit in coefficients, LDE and cap for every rate_bits 0..3 and both from_coeffs
    values at this log_n (tests/test_edge_values_cpu.py pins the oracle itself to Python integers for log_n 0..6 over
    the same rates).  rate_bits 0 and log_n 0, 1, 2 ran nowhere before."""
    n_polys = 3 if log_n in (10, 11) else 1
    case = 0
    for rate in range(4):
        for from_coeffs in (False, True):
            caps = [min(4, log_n + rate)]
            if log_n <= 3 and log_n + rate not in caps:
                caps.append(log_n + rate)                      # the leaf digests are the cap
            vals = _lde_input(log_n, n_polys, case + 8 * log_n)
            case += 1
            for cap in caps:
                co, lo, capo = oracle.lde_commit(vals, rate, cap, from_coeffs)
                cg, lg, capg = gpu.lde_commit(vals, rate, cap, from_coeffs)
                what = (log_n, rate, from_coeffs, cap)
                assert (cg == co).all(), what
                assert (lg == lo).all(), what
                assert (capg == capo).all(), what


@pytest.mark.parametrize("k,log_n,rate", [(0, 17, 0), (1, 17, 3), (2, 18, 0), (3, 18, 3), (4, 19, 0), (5, 19, 2),
                                          (6, 20, 0), (7, 20, 1)])
def test_factored_prescale_lde_vs_oracle(gpu, oracle, k, log_n, rate):
    """log_n 17..20 take the coset pre-scale as two factor tables (NTT_FACTOR_LOG in kernels_ntt.hip): before, that path
    ran only inside whole proofs, at rate 3, from values, where a wrong word would surface as "first differing proof
    word".  (20, 2) and (20, 3) cost the oracle most of a minute each and are left to the identity below."""
    from_coeffs = bool(k & 1)
    vals = _lde_input(log_n, 1, 200 + k)
    cap = 4
    co, lo, capo = oracle.lde_commit(vals, rate, cap, from_coeffs)
    cg, lg, capg = gpu.lde_commit(vals, rate, cap, from_coeffs)
    assert (cg == co).all() and (capg == capo).all()
    diff = np.nonzero(lg != lo)
    assert diff[0].size == 0, f"first differing LDE words {diff[1][:8].tolist()}"


@pytest.mark.parametrize("log_n", list(range(21)))
def test_lde_at_rate_r_begins_with_the_lde_at_rate_r_minus_1(gpu, log_n):
    """The first n << (r - 1) words of the bit-reversed LDE at rate r are the whole LDE at rate r - 1: with b = log_n + r
    and s = 1, position i' of the smaller one holds f(7 w_{b-1}^rev_{b-1}(i')), position i' of the larger one holds
    f(7 w_b^rev_b(i')), and for i' < 2^(b-1) rev_b(i') = 2 rev_{b-1}(i') -- rev_b(i' << s) = rev_(b-s)(i') read the other
    way round -- so the two points are the same.  No reference needed, so it runs at every log_n 0..20 and every rate
    >= 1, (20, 2) and (20, 3) included.  For those two shapes it covers ONLY the leading block: their other cosets (the
    trailing half of the LDE at each of the two rates) are compared with nothing."""
    vals = _lde_input(log_n, 1, 500 + log_n)
    from_coeffs = bool(log_n & 1)
    prev = None
    for rate in range(4):
        _c, lde, _cap = gpu.lde_commit(vals, rate, 0, from_coeffs)
        assert (lde < np.uint64(P)).all()
        if prev is not None:
            diff = np.nonzero(lde[:, :prev.shape[1]] != prev)
            assert diff[0].size == 0, f"log_n {log_n} rate {rate}: leading block differs from rate {rate - 1} at {diff[1][:8].tolist()}"
        prev = lde
