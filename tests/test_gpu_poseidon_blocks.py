"""GPU: the four-round partial blocks of the Poseidon permutation (plonky2.5_amd/csrc/poseidon_p3r.h).

Inside a permutation the blocks only ever see pseudo-random states, so tools/p4rcheck.hip (built by
__graft_entry__.build()) runs them where a fault would hide: each of the five blocks against the same four rounds one at
a time on all-ones words, boundary words and 4,096 random states; every table row with all the halves it multiplies at
0xFFFFFFFF (the bound the header's static_assert proves); the row reduction up to its precondition; the shared sum.
Then the library itself: p25_poseidon_permute on 4,096 boundary-valued states, and the smallest wide sponges that take
the trimmed row mask of the last absorbing permutation -- one 64-leaf workgroup of a 135-column matrix (7 words left:
rows 7..11) and of a 15-column one (7 left after one block) -- through p25_merkle_commit, against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import edge_values as ev
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_four_round_blocks_match_the_rounds_one_at_a_time():
    exe = os.path.join(ROOT, "tools", "build", "p4rcheck")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), "build/p4rcheck"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "P4RCHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
    for b in range(5):
        assert f"four_rounds block {b} (4177 states): 0 mismatches" in r.stdout, r.stdout[-2000:]
    for name in ("table rows at maximal halves", "reduce_row", "shared_sum"):
        assert any(line.startswith(name) and line.endswith(": 0 mismatches") for line in r.stdout.splitlines()), r.stdout[-2000:]


def test_permutation_on_boundary_valued_states(gpu, oracle):
    states = np.concatenate([ev.edge(2048 * 12, 1201), ev.mixed(1024 * 12, 1202), ev.high(512 * 12, 1203),
                             ev.low(512 * 12, 1204)]).reshape(4096, 12)
    got = gpu.poseidon_permute(states)
    want = oracle.poseidon_permute(states)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} states differ, first {bad[:4].tolist()}"


@pytest.mark.parametrize("width", [135, 15, 14, 13, 12, 11, 10, 9])   # 135 and 15 leave 7 words; 14 .. 9 leave 6 .. 1
def test_wide_sponge_with_a_partial_last_block(gpu, oracle, width):
    leaves = ev.mixed(64 * width, 1300 + width).reshape(64, width)
    cap_o, tree_o = oracle.merkle_commit(leaves, 0, want_tree=True)
    cap_g, tree_g = gpu.merkle_commit(np.ascontiguousarray(leaves.T), 0, want_tree=True)
    assert (tree_g.ravel() == tree_o.ravel()).all() and (cap_g == cap_o).all()
