"""CPU: the partial-round block tables of plonky2.5_amd/csrc/poseidon_p3r.h -- the head block and the five four-round
blocks, emulated on the host with the device's 32-bit-half accumulation -- against the round-by-round permutation on 10^5
random states, on boundary-valued states no permutation input can produce, block by block with the recorded deferred
offsets, and the coefficient sums that make the accumulation carry-free (tests/native/poseidon_blocks.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_block_tables_reproduce_the_round_by_round_permutation(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "poseidon_blocks")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "poseidon_blocks.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "POSEIDON BLOCKS OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
