"""CPU: the plain-Python plonky3 verifier (tests/p3_verify_model.py), the expected value of every p25_p3_verify_batch
test, pinned to the oracle.  The oracle has no plonky3 verifier; it holds the reference's in-circuit one: the witness of
Circuit.build_p3_verifier[_air](cfg) succeeds exactly when src/p3/verifier.rs accepts.  The model must accept and reject
what that witness accepts and rejects, on every single-word flip of five small shapes, and it must be able to return each
of its six codes."""
import numpy as np
import pytest

import p3_verify_cases as pc
import p3_verify_model as M


def test_model_accepts_the_artifact(p25, oracle, fib_inputs):
    assert M.verify(oracle, p25.Air.fibonacci(), p25.P3Config.fib64(), fib_inputs) == M.OK


# (family, log_blowup, quotient chunks)
FAMILIES = [("fib", 1, 1), ("tribonacci", 1, 1), ("squares", 1, 1), ("random_recurrence:1", 1, 1), ("random_recurrence:5", 1, 1),
            ("quadratic_pair:3", 1, 1), ("constant_pair", 1, 2), ("cubic", 1, 2), ("cubic_transition", 1, 2),
            ("fib", 2, 1), ("cubic", 2, 2), ("quartic_map:1", 2, 4), ("quintic_selector:2", 2, 4),
            ("squares", 3, 1), ("cubic_transition", 3, 2), ("quartic_map:6", 3, 4), ("sextic", 3, 8)]


@pytest.mark.parametrize("name,log_blowup,chunks", FAMILIES)
def test_model_accepts_host_proofs_of_every_family(p25, oracle, name, log_blowup, chunks):
    case = pc.Case(p25, name, 3, log_blowup, 2, 3)
    assert case.shape.Q == chunks
    assert M.verify(oracle, case.air, case.cfg, case.words) == M.OK
    assert pc.oracle_accepts(p25, oracle, case.air, case.cfg, case.words)
    # and the family's proof is not accepted whatever it holds: one flip in the opened values, one in the last path
    for pos in (case.shape.o_trace_local, case.shape.num_inputs - 1):
        bad = pc.flipped(case.words, pos)
        assert M.verify(oracle, case.air, case.cfg, bad) != M.OK
        assert not pc.oracle_accepts(p25, oracle, case.air, case.cfg, bad)


@pytest.mark.parametrize("key", pc.FLIP_SHAPES)
def test_every_single_word_flip_model_accepts_iff_the_oracle_does(p25, oracle, key):
    case = pc.flip_case(p25, key)
    assert case.words.size == {"fib_1_1_0": 58, "fib_2_2_3": 125, "fib_3_3_4": 240, "cubic": 175, "quartic_map": 231}[key]
    assert M.verify(oracle, case.air, case.cfg, case.words) == M.OK
    assert pc.oracle_accepts(p25, oracle, case.air, case.cfg, case.words)
    accepted = []
    for pos, proof in pc.all_flips(case.words):
        model_ok = M.verify(oracle, case.air, case.cfg, proof) == M.OK
        assert model_ok == pc.oracle_accepts(p25, oracle, case.air, case.cfg, proof), pos
        if model_ok:
            accepted.append(pos)
    # every flip is rejected but one: with pow_bits = 0 a flipped PoW witness still passes the check, and the one 2-bit
    # query index of that proof happens to stay the same
    assert accepted == ([36] if key == "fib_1_1_0" else [])


def test_flipped_pow_witness_without_pow_bits_is_accepted(p25, oracle):
    case = pc.flip_case(p25, "fib_1_1_0")
    assert case.shape.o_pow_witness == 36 and case.pow_bits == 0
    proof = pc.flipped(case.words, 36)
    assert M.verify(oracle, case.air, case.cfg, proof) == M.OK
    assert pc.oracle_accepts(p25, oracle, case.air, case.cfg, proof)


def test_a_second_valid_proof_is_accepted(p25, oracle):
    first = pc.flip_case(p25, pc.FIB334)
    second = pc.Case(p25, "fib", 3, 1, 3, 4, pow_start=12345)
    assert int(second.words[second.shape.o_pow_witness]) >= 12345 and not np.array_equal(first.words, second.words)
    assert M.verify(oracle, second.air, second.cfg, second.words) == M.OK
    assert pc.oracle_accepts(p25, oracle, second.air, second.cfg, second.words)


def test_model_yields_each_of_the_six_codes(p25, oracle):
    case = pc.flip_case(p25, pc.FIB334)
    seen = set()
    for name, (air, proof, code) in pc.code_cases(p25, oracle, case).items():
        assert M.verify(oracle, air, case.cfg, proof) == code, name
        if code != M.MALFORMED:      # a word >= p is no field element: the circuit's witness has no say on it
            assert not pc.oracle_accepts(p25, oracle, air, case.cfg, proof), name
        seen.add(code)
    assert seen == {M.MALFORMED, M.POW, M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY, M.CONSTRAINTS}


def test_model_precedence_on_double_tampers(p25, oracle):
    case = pc.flip_case(p25, pc.FIB334)
    for name, (air, proof, code) in pc.double_tampers(p25, case).items():
        assert M.verify(oracle, air, case.cfg, proof) == code, name
        if code != M.MALFORMED:
            assert not pc.oracle_accepts(p25, oracle, air, case.cfg, proof), name
