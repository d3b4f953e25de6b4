"""GPU: the levels of a Merkle tree above the leaf digests, in the forms a batch of proofs takes, against the oracle.

p25_merkle_commit and p25_merkle_commit_dev launch what a batch launches (kernels_hash.hip, launch_levels_to_cap): a
level with more than COOP_PARENTS_BATCH parents on k_tree_level at the batch wave priority, one parent per lane; a
smaller one on k_tree_level_coop, one parent per 16-lane group; and once a cap entry has at most TOP_MAX_NODES nodes
under it, k_tree_top_coop down to the cap in one launch.  The shapes below straddle those constants and the cap
heights; each compares the WHOLE tree (every level is read by the query kernel) and the cap with the oracle's, word
for word.  A leaf of at most four words is its own digest, so width 2 costs the oracle the tree's permutations only:
65 k for the largest shape.  The thresholds are read from the kernel source, so the shapes move with them.
Results do not depend on the wave priority, so this is regression coverage for launch_levels_to_cap, whatever priority
its levels run at.  (The fused k_tree_tail the module is named after was measured and not adopted:
tools/exp/tree_tail.patch; the shapes cover its block sizes too, should it return.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import splitmix_field
from device_buffers import Banded

pytestmark = pytest.mark.gpu


def _launch_constants():
    """The integer `constexpr` constants of kernels_hash.hip, read from the source so that the shapes follow them."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "plonky2.5_amd", "csrc", "kernels_hash.hip")
    vals = {}
    for line in open(src):
        m = re.match(r"constexpr\s+(?:int|size_t|unsigned|uint32_t)\s+([^;]+);", line)
        for name, expr in re.findall(r"(\w+)\s*=\s*([^,]+)", m.group(1)) if m else ():
            try:
                vals[name] = int(eval(expr, {"__builtins__": {}}, vals))
            except (NameError, SyntaxError, TypeError):
                pass                # not plain integer arithmetic: none of the constants used here
    return vals


_K = _launch_constants()
COOP_PARENTS_BATCH, TOP_MAX_NODES = _K["COOP_PARENTS_BATCH"], _K["TOP_MAX_NODES"]

SHAPES = [
    # (n_leaves, width, cap_height)
    (TOP_MAX_NODES, 7, 0),                  # exactly what the fused top takes: one launch above the leaves
    (2 * TOP_MAX_NODES, 2, 0),              # twice that: one cooperative level, then the top
    (2 * TOP_MAX_NODES, 7, 0),
    (128, 2, 0), (256, 7, 0), (512, 2, 0), (1024, 2, 0),
    (2 * COOP_PARENTS_BATCH, 2, 0),         # the first level has exactly COOP_PARENTS_BATCH parents: cooperative throughout
    (4 * COOP_PARENTS_BATCH, 2, 0),         # 4096 parents: one per-lane level at the batch priority, then cooperative ones
    (4 * COOP_PARENTS_BATCH, 7, 1),
    (4 * COOP_PARENTS_BATCH, 2, 4),
    (4 * COOP_PARENTS_BATCH, 7, 5),
    (4096, 7, 1), (4096, 2, 4), (4096, 7, 5),
    (2048, 2, 5),                           # 64 nodes per cap entry, 32 cap entries
    (1024, 7, 4),                           # 64 nodes per cap entry, 16 cap entries
    (1, 2, 0), (2, 7, 0),                   # n_leaves == cap (no launch above the leaves) and 2 * cap, cap_height 0
    (2, 2, 1), (4, 2, 1),                   # ... cap_height 1
    (16, 7, 4), (32, 2, 4),                 # ... cap_height 4
    (32, 2, 5), (64, 7, 5),                 # ... cap_height 5
    (1 << 15, 2, 0),                        # three per-lane levels, six cooperative ones, the top from 32 nodes
    (1 << 15, 2, 4),                        # the FRI tree of fib-64
    (1 << 16, 2, 4),                        # 2^16 leaves: four per-lane levels
    (1 << 16, 2, 1),
]
_IDS = [f"n{n}-w{w}-cap{c}" for n, w, c in SHAPES]

_reference = {}


def _case(oracle, n, w, cap):
    """(leaves row-major, oracle cap, oracle tree) of a shape: computed once, shared by the host and device cases."""
    key = (n, w, cap)
    if key not in _reference:
        leaves = splitmix_field(n * w, seed=7000 + 31 * n + 5 * w + cap).reshape(n, w)
        cap_o, tree_o = oracle.merkle_commit(leaves, cap, want_tree=True)
        for a in (leaves, cap_o, tree_o):
            a.setflags(write=False)
        _reference[key] = (leaves, cap_o, tree_o)
    return _reference[key]


def _first_diff(got, want):
    d = np.nonzero(got.ravel() != want.ravel())[0]
    return f"{d.size} words differ, first at {d[:8].tolist()}"


@pytest.mark.parametrize("n,w,cap", SHAPES, ids=_IDS)
def test_merkle_commit_tree_and_cap(gpu, oracle, n, w, cap):
    leaves, cap_o, tree_o = _case(oracle, n, w, cap)
    cap_g, tree_g = gpu.merkle_commit(np.ascontiguousarray(leaves.T), cap, want_tree=True)
    assert tree_g.size == tree_o.size == gpu.lib().p25_merkle_tree_words(n, cap)
    assert (tree_g.ravel() == tree_o.ravel()).all(), _first_diff(tree_g, tree_o)
    assert (cap_g.ravel() == cap_o.ravel()).all(), _first_diff(cap_g, cap_o)


@pytest.fixture(scope="module")
def side_stream(gpu):
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    yield s
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,w,cap", SHAPES, ids=_IDS)
def test_merkle_commit_dev_on_a_side_stream_with_guard_bands(gpu, oracle, side_stream, n, w, cap):
    """The device form on a stream of the caller's, the tree buffer between guard words: the tree equals the host
    form's and the oracle's, and no word before or behind it changed."""
    lib = gpu.lib()
    leaves, cap_o, tree_o = _case(oracle, n, w, cap)
    tw = int(lib.p25_merkle_tree_words(n, cap))
    cols = Banded(n * w, before=4097)
    tree = Banded(tw, before=4099)
    cols.set_async(np.ascontiguousarray(leaves.T), side_stream)        # the input arrives on the side stream too
    st = lib.p25_merkle_commit_dev(C.c_void_p(cols.ptr), n, n, w, cap, C.c_void_p(tree.ptr),
                                   C.c_void_p(side_stream.cuda_stream))
    assert st == 0, lib.p25_last_error().decode()
    side_stream.synchronize()
    got = tree.get()
    assert (got == tree_o.ravel()).all(), _first_diff(got, tree_o)
    assert (got[tw - (4 << cap):] == cap_o.ravel()).all()              # the cap is the tree's last 4 << cap words
    _cap_h, tree_h = gpu.merkle_commit(np.ascontiguousarray(leaves.T), cap, want_tree=True)
    assert (got == tree_h.ravel()).all(), _first_diff(got, tree_h)
    tree.assert_bands_intact()
    cols.assert_unchanged()
