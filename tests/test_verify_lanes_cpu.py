"""CPU: the verifier's per-lane functions (plonky2.5_amd/csrc/verify_lanes.h, ext_gates.h) compiled for the host and
run lane by lane in plain loops (tests/native/verify_lanes.cpp) against the oracle's verifier, with the oracle's proofs.

This is the arithmetic of three of the four GPU stages -- the vanishing identity with its gate evaluators in F_p^2, the
Merkle paths and the FRI query arithmetic, the verdict with its precedence -- without a GPU; the cooperative transcript
kernel and the launches themselves are covered by tests/test_gpu_verify.py.  The driver merges the lanes' keys in an
order that is not the verifier's, so a verdict that depended on which lane came last would show here.

The comparisons a flipped word never reaches -- openings against commitments, fold against next layer, the final
polynomial -- are reached by the forged proofs of tests/forged_proofs.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import forged_proofs as fp
import reference_vectors as rv
from conftest import ROOT, P
from verify_cases import (FRI_EVAL, FRI_MERKLE, INITIAL_MERKLE, MALFORMED, OK, POW, VANISHING, Layout, expected, flipped,
                          reference_gates_inputs)

CSRC = os.path.join(ROOT, "plonky2.5_amd", "csrc")


@pytest.fixture(scope="module")
def driver(p25, tmp_path_factory):
    p25.lib()                                   # libp25.so is there: the driver takes the circuit reader and the layout from it
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp("verify_lanes")
    exe = str(d / "verify_lanes")
    libdir = os.path.dirname(p25.binding.lib_path)
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "verify_lanes.cpp"),
                        "-o", exe, "-L" + libdir, "-lp25", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(c, dg, cap, proofs):
        blob, data = str(d / "circuit.blob"), str(d / "batch.bin")
        with open(blob, "wb") as f:
            f.write(c.to_blob())
        with open(data, "wb") as f:
            for part in (dg, cap, np.array([len(proofs)]), np.stack(proofs)):
                f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        r = subprocess.run([exe, blob, data], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]
    return run


class HostCase:
    """A circuit built on the host, the oracle's proof of it and the oracle's verifier data."""

    def __init__(self, oracle, c, inputs, seed):
        self.c, self.oc, self.inputs = c, oracle.load_circuit(c.to_blob()), np.asarray(inputs, dtype=np.uint64)
        self.proof, st, _t, msg = self.oc.prove(self.inputs, seed=seed)
        assert st == 0, msg
        self.dg, self.cap = self.oc.digest()
        self.L = Layout(c)

    def parity(self, driver, proofs):
        got = driver(self.c, self.dg, self.cap, proofs)
        want = [expected(self.oc, p, self.dg, self.cap) for p in proofs]
        assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
        return want


@pytest.fixture(scope="module")
def and_case(p25, oracle):
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    return HostCase(oracle, p25.Circuit.build_gadget(0, 0), [x, y, (x & y) % P], seed=5)


@pytest.fixture(scope="module")
def rec_case(p25, oracle, and_case):
    outer = and_case.c.build_recursive_verifier(1, and_case.dg, and_case.cap)     # verifier data given: host-only
    return HostCase(oracle, outer, and_case.proof, seed=1)


def test_lanes_accept_the_reference_gates_and_public_inputs(p25, oracle, driver):
    xs = [(0x9E3779B97F4A7C15 * (i + 1)) % P for i in range(3)]
    for kind, param, inputs in ((11, 3, xs), (12, 0, [rv.INTERLEAVE_X]), (13, 0, [rv.UNINTERLEAVE_X]),
                                (14, 0, reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF)),
                                (6, 19, [5, 7 * pow(pow(1753635133440165772, 1 << 13, P), 5, P) % P])):
        case = HostCase(oracle, p25.Circuit.build_gadget(kind, param), inputs, seed=3)
        assert case.parity(driver, [case.proof]) == [OK], kind


def test_lanes_single_word_tamper_parity_and_gadget(and_case, driver):
    words = list(range(0, and_case.proof.size, 29)) + [626, 627]
    want = and_case.parity(driver, [and_case.proof] + [flipped(and_case.proof, w) for w in words])
    assert set(want) == {OK, VANISHING, POW, INITIAL_MERKLE} and want[-2:] == [POW, POW]


def test_lanes_single_word_tamper_parity_with_fri_layers(rec_case, driver):
    words = list(range(0, rec_case.proof.size, 41 * 3))
    want = rec_case.parity(driver, [rec_case.proof] + [flipped(rec_case.proof, w) for w in words])
    assert set(want) == {OK, VANISHING, POW, INITIAL_MERKLE, FRI_EVAL, FRI_MERKLE}


def test_lanes_precedence_and_wrong_verifier_data(rec_case, driver):
    L, proof = rec_case.L, rec_case.proof
    pair = [flipped(proof, L.sibling(5, 4, 1), L.leaf(9, 1, 3)), flipped(proof, L.leaf(5, 1, 3), L.sibling(9, 4, 1))]
    assert rec_case.parity(driver, pair) == [FRI_MERKLE, INITIAL_MERKLE]
    dg = rec_case.dg.copy()
    dg[2] ^= np.uint64(1)
    assert driver(rec_case.c, dg, rec_case.cap, [proof]) == [VANISHING] == [expected(rec_case.oc, proof, dg, rec_case.cap)]
    cap = rec_case.cap.copy()
    cap[:, 0] ^= np.uint64(1)
    assert driver(rec_case.c, rec_case.dg, cap, [proof]) == [INITIAL_MERKLE] == [expected(rec_case.oc, proof, rec_case.dg, cap)]


def test_lanes_reject_words_at_or_above_p(and_case, driver):
    L, proof = and_case.L, and_case.proof
    batch = [proof]
    for pos in (L.zs_cap + 5, L.wires + 3, L.leaf(0, 0, 2), L.final_poly + 1):
        for word in (P, (1 << 64) - 1, P + 5):
            q = proof.copy()
            q[pos] = np.uint64(word)
            batch += [q, proof]
    assert driver(and_case.c, and_case.dg, and_case.cap, batch) == [OK] + [MALFORMED, OK] * 12


@pytest.mark.parametrize("which", ["and_case", "rec_case"])
def test_lanes_answer_forged_proofs_with_the_tables_codes(request, driver, which):
    """Proofs that fail exactly one check (tests/forged_proofs.py), among honest ones: the verdicts are the table's, which
    are the oracle's, and every honest neighbour is accepted."""
    case = request.getfixturevalue(which)
    forged = fp.forge(case.oc, case.c, case.inputs)
    assert fp.oracle_codes(case.oc, forged, case.dg, case.cap) == [f.code for f in forged]
    batch, want, names = fp.mixed(forged, case.proof, seed=len(forged))
    got = driver(case.c, case.dg, case.cap, list(batch))
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert set(want) == ({OK, VANISHING, FRI_EVAL, fp.FINAL_POLY} if case.L.n_layers else {OK, VANISHING, fp.FINAL_POLY})
