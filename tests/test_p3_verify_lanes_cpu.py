"""CPU: the plonky3 verifier's per-lane functions (plonky2.5_amd/csrc/p3_verify_lanes.h) compiled for the host and run
lane by lane in plain loops (tests/native/p3_verify_lanes.cpp) against the model (tests/p3_verify_model.py).

This is the arithmetic of four of the five GPU stages -- the identity with the AIR interpreter in F_p^2, the reduced
openings and fold chains, the Merkle paths, the verdict with its precedence -- and the plain statement of the transcript,
without a GPU; the cooperative transcript kernel and the launches are covered by tests/test_gpu_p3_verify.py.  The driver
merges the lanes' keys in an order that is not the verifier's, so a verdict that depended on which lane came last would
show here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import p3_verify_cases as pc
import p3_verify_model as M
from conftest import ROOT, P

CSRC = os.path.join(ROOT, "plonky2.5_amd", "csrc")


def _build_driver(p25, tmp_path_factory, name, extra):
    p25.lib()                                   # libp25.so is there: the driver takes the AIR's compilation and the shape from it
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp(name)
    exe = str(d / "p3_verify_lanes")
    libdir = os.path.dirname(p25.binding.lib_path)
    r = subprocess.run([gxx, "-std=c++17", "-O1"] + extra + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "p3_verify_lanes.cpp"),
                        "-o", exe, "-L" + libdir, "-lp25", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(case, proofs, air=None):
        air = air or case.air
        data = str(d / "batch.bin")
        head = [air.width, len(air.nodes), len(air.constraints), case.log_n, case.log_blowup, case.queries, case.pow_bits, len(proofs)]
        with open(data, "wb") as f:
            for part in (head, [x for nd in air.nodes for x in nd], [x for c in air.constraints for x in c], np.stack(proofs)):
                f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]
    return run


@pytest.fixture(scope="module")
def driver(p25, tmp_path_factory):
    return _build_driver(p25, tmp_path_factory, "p3_verify_lanes", [])


@pytest.fixture(scope="module")
def sanitized_driver(p25, tmp_path_factory):
    """The same stand-alone program with the lane functions under AddressSanitizer and UBSan (host code, CPU only)."""
    return _build_driver(p25, tmp_path_factory, "p3_verify_lanes_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_lanes_equal_the_model_on_every_flip(p25, oracle, driver):
    case = pc.flip_case(p25, pc.FIB334)
    proofs = [case.words] + [w for _pos, w in pc.all_flips(case.words)]
    want = [M.verify(oracle, case.air, case.cfg, w) for w in proofs]
    got = driver(case, proofs)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    assert want[0] == M.OK and set(want[1:]) == {M.POW, M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY}


def test_lanes_the_six_codes_and_precedence(p25, oracle, driver):
    case = pc.flip_case(p25, pc.FIB334)
    cases = dict(pc.code_cases(p25, oracle, case))
    cases.update(pc.double_tampers(p25, case))
    for name, (air, proof, code) in cases.items():
        assert M.verify(oracle, air, case.cfg, proof) == code, name
        assert driver(case, [proof, case.words], air=air) == [code, M.CONSTRAINTS if air is not case.air else M.OK], name


@pytest.mark.parametrize("name,log_blowup", [("cubic", 1), ("quartic_map:6", 2), ("sextic", 3), ("random_recurrence:5", 1)])
def test_lanes_accept_more_chunks_and_flips_match(p25, oracle, driver, name, log_blowup):
    case = pc.Case(p25, name, 3, log_blowup, 2, 3)
    flips = pc.all_flips(case.words)[::7]
    proofs = [case.words] + [w for _pos, w in flips]
    want = [M.verify(oracle, case.air, case.cfg, w) for w in proofs]
    assert want[0] == M.OK and M.OK not in want[1:]
    assert driver(case, proofs) == want


def test_lanes_reject_words_at_or_above_p(p25, driver):
    case = pc.flip_case(p25, pc.FIB334)
    s = case.shape
    batch = [case.words]
    for pos in (2, s.o_chunks + 1, s.step(1, 2) + 3, s.o_pow_witness, s.num_inputs - 1):
        for word in (P, (1 << 64) - 1, P + 5):
            batch += [pc.with_word(case.words, pos, word), case.words]
    assert driver(case, batch) == [M.OK] + [M.MALFORMED, M.OK] * 15


def test_lanes_stay_in_bounds_under_the_sanitizers(p25, oracle, sanitized_driver):
    """Every index the lanes form comes from the shape or from a masked query index: whatever the proof holds -- all flips,
    words of all ones, all zeros, eight chunks, width 64 at the smallest height -- the sanitized driver runs clean (a report
    ends it with a non-zero status) and prints the model's verdicts."""
    case = pc.flip_case(p25, pc.FIB334)
    ones = np.full(case.words.size, (1 << 64) - 1, dtype=np.uint64)
    proofs = [case.words] + [w for _pos, w in pc.all_flips(case.words)] + [ones, np.zeros_like(ones)]
    assert sanitized_driver(case, proofs) == [M.verify(oracle, case.air, case.cfg, w) for w in proofs]
    for name, log_n, log_blowup, queries, pow_bits in (("sextic", 3, 3, 2, 3), ("random_recurrence:64", 1, 1, 1, 0)):
        case = pc.Case(p25, name, log_n, log_blowup, queries, pow_bits)
        proofs = [case.words] + [w for _pos, w in pc.all_flips(case.words)][::5]
        assert sanitized_driver(case, proofs) == [M.verify(oracle, case.air, case.cfg, w) for w in proofs]
