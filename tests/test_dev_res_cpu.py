"""CPU: the owners of the library's device buffers, events and streams (plonky2.5_amd/csrc/dev_res.h), checked by a plain C++
program (tests/native/dev_res.cpp) against a counting test double of the HIP runtime (tests/native/fake_hip): release exactly
once, moves, regrow, and a constructor that fails at each of its creations in turn.  Built twice: plain, and with the address
and undefined-behaviour sanitizers (run directly; skipped where their runtime is not installed)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def _build(tmp_path, name, extra):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    r = subprocess.run([gxx, "-std=c++17", "-Wall", *extra, "-I" + os.path.join(ROOT, "tests", "native", "fake_hip"),
                        "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"), os.path.join(ROOT, "tests", "native", "dev_res.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    return exe, r


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEV_RES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_owners_release_once_move_regrow_and_unwind(tmp_path):
    exe, r = _build(tmp_path, "dev_res", ["-O2"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    _run(exe)


def test_owners_under_address_and_undefined_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "dev_res_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and "cannot find" in r.stderr:   # the linker, of libasan / libubsan
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    _run(exe)
