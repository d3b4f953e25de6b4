"""CPU: how many proofs a circuit keeps in flight and which proving context takes which proof (plonky2.5_amd/csrc/inflight.h).
The assignment is checked by a plain C++ program (tests/native/inflight.cpp); p25_runtime_info reports the stream pool as it
is -- 16 wide before any circuit has proved -- whatever hardware-queue count the environment names."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


def test_context_assignment_is_balanced_over_every_window(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "inflight")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "inflight.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "INFLIGHT OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import __graft_entry__ as ge
p25 = ge.load_package()
ri = p25.runtime_info().as_dict()
c = p25.Circuit.build_gadget(0, 0)          # host tables only: no device use, no proving context
ri2 = p25.runtime_info().as_dict()
print("RI", ri["proving_streams"], ri["main_streams"], ri["hw_queues_env"], ri2["proving_streams"])
"""


@pytest.mark.parametrize("queues", [None, "1", "2", "4", "8", "32"])
def test_runtime_info_reports_16_proving_streams_before_any_circuit_proves(queues):
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RI ")][0].split()
    assert line[1:] == ["16", "2", queues or "0", "16"], line
