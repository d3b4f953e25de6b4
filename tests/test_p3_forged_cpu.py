"""CPU: the plonky3 verifiers on forged proofs from a model prover, and the host prover against that model.

tests/p3_prove_model.py states in Python integers, without a transform, what p25_p3_prove_air_ax must write;
tests/p3_forged_cases.py forges with it the proofs a cheating prover would send -- finished honestly from faulted data, so
that exactly one check fails -- and writes the expected code of each down from the documented order of checks.

1. the model prover's words ARE the host prover's, shape by shape (the host prover is the yardstick of the device prover)
2. every forged proof: the verifier model gives the table's code; the oracle's witness of the reference's verifier circuit
   refuses it and accepts the honest proof
3. the device verifier's lane functions, compiled for the host (plain, and under ASan / UBSan), on the mixed batches
4. precedence of two failures, one expectation each
5. the trace checker names the constraint and row the fault broke; the host prover refuses that trace
Every comparison is equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import p3_aux_model as M
import p3_check_model as CK
import p3_forged_cases as FC
import p3_prove_model as PV
import p3_verify_model
from conftest import ROOT

INVALID_ARG, WITNESS_CONFLICT = 1, 4
PLAIN = ("fib", "cubic", "quartic_map")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module", params=FC.SHAPE_IDS)
def built(request, p25, oracle):
    return FC.build(p25, oracle, request.param)


def _cfg(p25, b):
    return p25.P3Config(*[getattr(b.cfg, f) for f in PV.Config.FIELDS])


# ---- 1. the model prover is the host prover -----------------------------------------------------------------------------
def test_the_model_prover_is_the_host_prover(p25, built):
    b = built
    want, cfg = p25.p3_prove_air(b.air, b.trace, num_queries=b.queries, pow_bits=b.pow_bits, pow_start=b.pow_start, threads=1,
                                 log_blowup=b.log_blowup, public_values=b.pv)
    assert b.cfg.same_as(cfg)
    assert np.array_equal(b.words, want)


@pytest.mark.parametrize("name,pow_start", [("fib", 1000), ("range", 77), ("perm_b2", (1 << 40) + 3)])
def test_the_model_prover_is_the_host_prover_from_another_pow_start(p25, oracle, name, pow_start):
    b = FC.build(p25, oracle, name)
    got = PV.prove(oracle, b.air, b.trace, b.log_blowup, b.queries, b.pow_bits, pow_start, b.pv)
    want, _cfg = p25.p3_prove_air(b.air, b.trace, num_queries=b.queries, pow_bits=b.pow_bits, pow_start=pow_start, threads=1,
                                  log_blowup=b.log_blowup, public_values=b.pv)
    assert got.pow_witness >= pow_start and np.array_equal(got.words, want)


@pytest.mark.parametrize("name,log_n,log_blowup", [("sextic", 3, 3), ("fib", 1, 1), ("fib", 4, 3)])
def test_the_model_prover_is_the_host_prover_at_eight_chunks_and_the_smallest_height(p25, oracle, name, log_n, log_blowup):
    import p3_verify_cases as pc
    air, trace = pc.air_and_trace(p25, name, log_n)
    got = PV.prove(oracle, air, trace, log_blowup, 2, 3, 0)
    want, cfg = p25.p3_prove_air(air, trace, num_queries=2, pow_bits=3, pow_start=0, threads=1, log_blowup=log_blowup)
    assert got.cfg.same_as(cfg) and np.array_equal(got.words, want)


# ---- 2. the model verifier and the oracle's circuit on every forged proof ------------------------------------------------
def test_the_set_holds_what_the_table_lists(built):
    b = built
    kinds = {f.kind for f in b.forged}
    assert {"row", "chunk", "fold", "opened", "final"} <= kinds
    assert ("unbalanced" in kinds) == ("aux_start" in kinds) == bool(b.shape.AW)
    assert {f.code for f in b.forged} == {M.FRI_MERKLE, M.FINAL_POLY, M.CONSTRAINTS}
    assert len({f.proof.tobytes() for f in b.forged} | {b.words.tobytes()}) == len(b.forged) + 1
    for f in b.forged:
        if f.kind == "opened":                               # the precondition, asserted
            assert any(i >> b.log_n for i in f.indices), f.name


def test_the_model_verifier_gives_the_tables_code(oracle, built):
    b = built
    assert b.verify(oracle, b.words) == M.OK
    for f in b.forged:
        assert b.verify(oracle, f.proof) == f.code, f.name
        if b.name in PLAIN:
            assert p3_verify_model.verify(oracle, b.air, b.cfg, f.proof) == f.code, f.name


def test_the_oracles_verifier_circuit_refuses_every_forged_proof(p25, oracle, built):
    b = built
    oc = oracle.load_circuit(p25.Circuit.build_p3_verifier_air(_cfg(p25, b), b.air).to_blob())
    assert oc.witness(b.words)[1] == 0
    for f in b.forged:
        assert oc.witness(f.proof)[1] == WITNESS_CONFLICT, f.name


# ---- 3, 4. the lane functions on the host ---------------------------------------------------------------------------------
def _compile(p25, d, source, extra):
    p25.lib()
    gxx = shutil.which("g++")
    assert gxx, "g++ not available"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    exe = str(d / (source[:-4] + ("_san" if extra else "")))
    libdir = os.path.dirname(p25.binding.lib_path)
    r = subprocess.run([gxx, "-std=c++17", "-O1"] + extra + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                        "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "native", source), "-o", exe, "-L" + libdir, "-lp25",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def lanes(p25, tmp_path_factory):
    """run(b, proofs, sanitized) -> verdicts: tests/native/p3_verify_lanes.cpp for the plain shapes, p3_verify_lanes_aux.cpp
    in its `full` form for the others; both stand-alone programs, each built plain and under ASan / UBSan."""
    d = tmp_path_factory.mktemp("p3_forged_lanes")
    exes = {(src, bool(extra)): _compile(p25, d, src, extra)
            for src in ("p3_verify_lanes.cpp", "p3_verify_lanes_aux.cpp") for extra in ([], SANITIZE)}

    def run(b, proofs, sanitized):
        air, data = b.air, str(d / "batch.bin")
        head = [air.width, len(air.nodes), len(air.constraints), b.log_n, b.log_blowup, b.queries, b.pow_bits, len(proofs)]
        parts = [[x for nd in air.nodes for x in nd], [x for c in air.constraints for x in c]]
        if b.name in PLAIN:
            cmd = [exes[("p3_verify_lanes.cpp", sanitized)], data]
        else:
            cmd = [exes[("p3_verify_lanes_aux.cpp", sanitized)], data, "full"]
            head += [air.n_challenges, len(air.aux_columns), air.n_public, len(air.periodic_columns), b.shape.PW, 0]
            parts.append([x for c in air.aux_columns for x in c])
            for col in air.periodic_columns:
                parts += [[int(col.size).bit_length() - 1], col]
            if b.shape.PW:
                parts += [air.preprocessed, b.prep_commit]
        with open(data, "wb") as f:
            for part in [head] + parts + [np.stack(proofs)]:
                f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]
    return run


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_lanes_give_the_tables_codes_on_the_mixed_batch(built, lanes, sanitized):
    b = built
    batch, want, names = FC.mixed(b.forged, b.words, seed=11)
    got = lanes(b, list(batch), sanitized)
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert {0, M.FRI_MERKLE, M.FINAL_POLY, M.CONSTRAINTS} <= set(want)


@pytest.mark.parametrize("name", ["fib", "range"])
def test_precedence_of_two_failures(p25, oracle, lanes, name):
    b = FC.build(p25, oracle, name)
    cases = FC.precedence(b)
    assert [c for _p, c in cases.values()] == [M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY, M.MALFORMED, M.FRI_MERKLE, M.FINAL_POLY]
    for label, (proof, code) in cases.items():
        assert b.verify(oracle, proof) == code, label
    proofs = [p for p, _c in cases.values()]
    for sanitized in (False, True):
        assert lanes(b, proofs + [b.words], sanitized) == [c for _p, c in cases.values()] + [0]


# ---- 5. the checker says where, the prover refuses --------------------------------------------------------------------------
def _first_with_sums_from_one(oracle, b, f):
    """aux_start: the first (row, constraint) the AIR's constraints miss when column j starts at 1, from the definition."""
    chal = M.challenges_of(oracle, b.air, f.proof, b.cfg, b.prep_commit)
    pv = [int(v) for v in f.pv] if f.pv is not None else []
    sums = M.running_sums(b.air, f.trace, pv, chal)
    sums = [[M.e_add(v, M.e(1)) if j == f.fault[1] else v for j, v in enumerate(row)] for row in sums]
    n = len(sums)
    rows = [[M.e(int(x)) for x in r] for r in f.trace]
    prep = None if b.air.preprocessed is None else [[M.e(int(x)) for x in r] for r in b.air.preprocessed]
    for i in range(n):
        i1 = (i + 1) % n
        per = [M.e(int(c[i % len(c)])) for c in b.air.periodic_columns]
        v = M.eval_nodes(b.air, rows[i], rows[i1], pv, per, prep[i] if prep else None, prep[i1] if prep else None, chal,
                         sums[i], sums[i1])
        for c, (node, when) in enumerate(b.air.constraints):
            if CK.selected(when, i, n) and v[node] != M.e(0):
                return (i, c)
    return None


def test_the_checker_names_what_the_fault_broke_and_the_prover_refuses(p25, oracle, built):
    b = built
    seen = 0
    for f in b.forged:
        if f.kind == "aux_start":                            # the column is the prover's to build: the trace itself is honest
            assert _first_with_sums_from_one(oracle, b, f) == f.first, f.name
            assert p25.p3_check_air(b.air, f.trace, f.pv, b.log_blowup, threads=1).verdict == CK.OK
            continue
        if f.kind not in ("row", "unbalanced", "public"):
            assert f.first is None
            continue
        seen += 1
        want = CK.report(oracle, p25, b.air, f.trace, f.pv, b.log_blowup)
        assert (want[0], want[2], want[3]) == (CK.VIOLATED,) + f.first, f.name
        rep = p25.p3_check_air(b.air, f.trace, f.pv, b.log_blowup, threads=1)
        assert rep.words == want and rep.first == f.first, f.name
        with pytest.raises(p25.P25Error) as ei:
            p25.p3_prove_air(b.air, f.trace, num_queries=b.queries, pow_bits=b.pow_bits, threads=1, log_blowup=b.log_blowup,
                             public_values=f.pv)
        assert ei.value.status == INVALID_ARG, f.name
    assert seen >= 2
    assert {f.first[1] for f in b.forged if f.first} >= {0}          # the constraint under the highest alpha power


def test_the_faults_reach_every_kind_of_constraint_and_both_ends_of_the_fold(p25):
    """Over the shapes: a first-row, a transition, a last-row and an always constraint is reported first; in every shape the
    constraint under the highest power of alpha is, and in most the one under the lowest."""
    whens, lowest = set(), 0
    for name, spec in FC.SPECS.items():
        air = spec.make(p25)[0]
        firsts = [first for _rc, first in spec.rows] + [first for _i, first in spec.public] + [first for _j, first in spec.aux_start]
        firsts += [spec.unbalanced[1]] if spec.unbalanced else []
        assert 0 in {c for _r, c in firsts}, name
        whens |= {air.constraints[c][1] for _r, c in firsts}
        lowest += any(c == len(air.constraints) - 1 for _r, c in firsts)
    assert whens == {0, 1, 2, 3} and lowest >= len(FC.SPECS) - 1
