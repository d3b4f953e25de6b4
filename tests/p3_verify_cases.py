"""Inputs of the plonky3 verifier's tests (p25_p3_verify_batch): proofs of small shapes, the tampers that reach each
verdict and the oracle's word on a proof -- the witness of the reference's in-circuit verifier, which succeeds exactly
when src/p3/verifier.rs accepts.  Expected verdicts come from tests/p3_verify_model.py."""
import numpy as np

import air_cases
import p3_verify_model as M

P = M.P
# the shapes of the flip sweep: name -> (air maker, trace maker, log_n, log_blowup, queries, pow_bits)
FLIP_SHAPES = ("fib_1_1_0", "fib_2_2_3", "fib_3_3_4", "cubic", "quartic_map")
FIB334 = "fib_3_3_4"


def sextic(p25):
    """width 2, degree 6 in an ALWAYS constraint (EIGHT quotient chunks, needs log_blowup 3): y = x^6 + 3 on every row;
    next x = y + 1; first row x = 2."""
    air = p25.Air(2)
    x, y = air.local(0), air.local(1)
    x2 = air.mul(x, x)
    air.assert_zero(air.sub(air.add(air.mul(air.mul(x2, x2), x2), air.const(3)), y))
    air.when_first_row(air.sub(x, air.const(2)))
    air.when_transition(air.sub(air.next(0), air.add(y, air.const(1))))
    return air


def sextic_trace(log_n):
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    x = 2
    for i in range(1 << log_n):
        y = (pow(x, 6, P) + 3) % P
        t[i] = (x, y)
        x = (y + 1) % P
    return t


def air_and_trace(p25, name, log_n):
    """The families of tests/air_cases.py (and `sextic`) by name -> (air, trace)."""
    if name == "fib":
        return p25.Air.fibonacci(), air_cases.fib_trace(log_n)
    if name == "tribonacci":
        return air_cases.tribonacci(p25), air_cases.tribonacci_trace(log_n)
    if name == "squares":
        return air_cases.squares(p25), air_cases.squares_trace(log_n)
    if name == "cubic":
        return air_cases.cubic(p25), air_cases.cubic_trace(log_n)
    if name == "cubic_transition":
        return air_cases.cubic_transition(p25), air_cases.cubic_transition_trace(log_n)
    if name == "sextic":
        return sextic(p25), sextic_trace(log_n)
    if name == "constant_pair":
        return air_cases.constant_pair(p25, 1), air_cases.constant_pair_trace(1, log_n)
    fam, arg = name.rsplit(":", 1)
    if fam == "random_recurrence":                      # random_recurrence:<width>, seed 7
        air, coef = air_cases.random_recurrence(p25, 7, int(arg))
        return air, air_cases.random_recurrence_trace(coef, log_n)
    make, trace = {"quadratic_pair": (air_cases.quadratic_pair, air_cases.quadratic_pair_trace),
                   "quartic_map": (air_cases.quartic_map, air_cases.quartic_map_trace),
                   "quintic_selector": (air_cases.quintic_selector, air_cases.quintic_selector_trace)}[fam]
    air, par = make(p25, int(arg))                      # <family>:<seed>
    return air, trace(par, log_n)


class Case:
    """A valid proof: its AIR, words, P3Config and layout (p3_verify_model.Shape)."""

    def __init__(self, p25, name, log_n, log_blowup, queries, pow_bits, pow_start=0):
        self.name, self.log_n, self.log_blowup, self.queries, self.pow_bits = name, log_n, log_blowup, queries, pow_bits
        self.air, self.trace = air_and_trace(p25, name, log_n)
        self.words, self.cfg = p25.p3_prove_air(self.air, self.trace, num_queries=queries, pow_bits=pow_bits,
                                                pow_start=pow_start, threads=1, log_blowup=log_blowup)
        self.shape = M.Shape(self.cfg)
        assert self.words.size == self.shape.num_inputs

    def prover(self, p25, air=None):
        return p25.P3Prover(air or self.air, self.log_n, self.log_blowup, self.queries, self.pow_bits)


_cases = {}


def flip_case(p25, key):
    if key not in _cases:
        _cases[key] = {"fib_1_1_0": lambda: Case(p25, "fib", 1, 1, 1, 0), "fib_2_2_3": lambda: Case(p25, "fib", 2, 1, 2, 3),
                       "fib_3_3_4": lambda: Case(p25, "fib", 3, 1, 3, 4), "cubic": lambda: Case(p25, "cubic", 3, 1, 2, 3),
                       "quartic_map": lambda: Case(p25, "quartic_map:6", 3, 2, 2, 3)}[key]()
    return _cases[key]


def flipped(words, *positions):
    """A copy with bit 0 of the words at `positions` flipped."""
    w = np.array(words, dtype=np.uint64)
    for p in positions:
        w[p] ^= np.uint64(1)
    return w


def all_flips(words):
    """[(position, proof)] for every single-word flip that keeps the word below p."""
    return [(i, flipped(words, i)) for i in range(len(words)) if (int(words[i]) ^ 1) < P]


def with_word(words, pos, value):
    w = np.array(words, dtype=np.uint64)
    w[pos] = np.uint64(value)
    return w


_circuits = {}


def oracle_accepts(p25, oracle, air, cfg, words):
    """The reference's in-circuit verifier for (air, cfg) on the proof: True iff its witness generation succeeds."""
    key = (air.width, tuple(air.nodes), tuple(air.constraints), bytes(cfg))
    if key not in _circuits:
        _circuits[key] = oracle.load_circuit(p25.Circuit.build_p3_verifier_air(cfg, air).to_blob())
    return _circuits[key].witness(np.asarray(words, dtype=np.uint64))[1] == 0


def wrong_air(p25):
    """A DIFFERENT width-3 AIR with one quotient chunk: a Fibonacci proof has its shape and fails only its identity."""
    return air_cases.squares(p25)


def pow_tamper(oracle, case):
    """The first trace-root word whose flip the model rejects at the proof of work (deterministic for the fixed proof; 15
    flips in 16 do at 4 bits)."""
    for pos in range(4):
        if M.verify(oracle, case.air, case.cfg, flipped(case.words, pos)) == M.POW:
            return pos
    raise AssertionError("no trace-root flip fails the proof of work")


def code_cases(p25, oracle, case):
    """name -> (air, proof, code): the tamper of the issue's table for each of the six codes, on a Fibonacci proof."""
    s, w = case.shape, case.words
    return {
        "malformed": (case.air, with_word(w, s.o_trace_next + 1, P), M.MALFORMED),
        "pow": (case.air, flipped(w, pow_tamper(oracle, case)), M.POW),
        "input_row": (case.air, flipped(w, s.opening(1, 0) + 2), M.INPUT_MERKLE),
        "input_path": (case.air, flipped(w, s.opening(0, 1) + 2 * s.Q + 5), M.INPUT_MERKLE),
        "fri_sibling": (case.air, flipped(w, s.step(1, 1)), M.FRI_MERKLE),
        "fri_path": (case.air, flipped(w, s.step(2, 0) + 2 + 3), M.FRI_MERKLE),
        "final_poly": (case.air, flipped(w, s.o_final_poly + 1), M.FINAL_POLY),
        "constraints": (wrong_air(p25), np.array(w), M.CONSTRAINTS),
    }


def double_tampers(p25, case):
    """name -> (air, proof, code): two failures in one proof, the verdict is the earlier one's."""
    s, w = case.shape, case.words
    fp = s.o_final_poly
    return {
        "q2 input path + final_poly": (case.air, flipped(w, s.opening(2, 0) + s.W + 1, fp), M.INPUT_MERKLE),
        "q1 FRI sibling + final_poly": (case.air, flipped(w, s.step(1, 0), fp), M.FINAL_POLY),      # query 0's comparison first
        "q0 FRI round-1 path + final_poly": (case.air, flipped(w, s.step(0, 1) + 2, fp), M.FRI_MERKLE),
        "word = p + final_poly": (case.air, with_word(flipped(w, fp), s.opening(1, 1), P), M.MALFORMED),
        "word = p + FRI sibling": (case.air, with_word(flipped(w, s.step(0, 0)), 3, P), M.MALFORMED),
        "wrong AIR + final_poly": (wrong_air(p25), flipped(w, fp), M.FINAL_POLY),
    }
