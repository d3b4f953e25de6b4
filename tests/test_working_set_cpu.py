"""CPU: the prover's sizing, stated once (plonky2.5_amd/csrc/prover_shape.h, working_set.h), checked by a plain C++ program
(tests/native/working_set.cpp) against the counting test double of the HIP runtime (tests/native/fake_hip) over a grid of
circuit shapes from 2^2 to 2^19 rows: a context requests exactly the bytes the free-memory clamp counts for it, one
allocation per line of the table; every buffer has the words the constructor gave it before there was a table (restated
in the program, one line per buffer); a construction that fails at any of its creations gives everything back; the
stand-alone FRI proof's layout is the one stated there in numbers.  Built twice: plain, and with the address and
undefined-behaviour sanitizers (run directly; skipped where their runtime is not installed).  The double's hipMalloc is a
real malloc, so the sanitizer run sizes every shape of the grid but constructs the contexts of up to 8 MiB only."""
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
                        "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"), os.path.join(ROOT, "tests", "native", "working_set.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    return exe, r


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])   # the context bytes of the fib-64 and the config-5 circuit, by the old formula and exact
    assert r.returncode == 0 and "WORKING_SET OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_working_set_matches_its_table_and_unwinds(tmp_path):
    exe, r = _build(tmp_path, "working_set", ["-O2"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    out = _run(exe)
    assert "1260 shapes sized, 1260 of them constructed" in out


def test_working_set_under_address_and_undefined_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "working_set_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and "cannot find" in r.stderr:   # the linker, of libasan / libubsan
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    out = _run(exe, str(8 << 20))
    assert "1260 shapes sized, 324 of them constructed" in out
