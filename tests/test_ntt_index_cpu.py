"""CPU: the index maps of the NTT tile kernel (plonky2.5_amd/csrc/ntt_index.h) -- the cursors the kernel advances from
element to element against the closed forms of the addressing kinds, for every form, every sub-transform length and tile
width and both block sizes; each block's load and store maps are bijections onto its LDS slots, and the blocks of a launch
cover the polynomial once.  Checked by a plain C++ program (tests/native/ntt_index.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_ntt_cursors_equal_the_closed_forms_and_tile_the_polynomial(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "ntt_index")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "ntt_index.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NTT INDEX OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
