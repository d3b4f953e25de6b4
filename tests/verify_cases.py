"""What the verifier tests share (tests/test_gpu_verify.py on the GPU, tests/test_verify_lanes_cpu.py on the host): the
verdict codes, the oracle as the yardstick, single-word tampers, and the flat proof's layout computed from
p25_circuit_info and the layout comment in include/p25.h."""
import numpy as np

P = 0xFFFFFFFF00000001
OK, INVALID_ARG = 0, 1
VANISHING, POW, MALFORMED, INITIAL_MERKLE, FRI_EVAL, FRI_MERKLE, FINAL_POLY = range(20, 27)
CAP_WORDS, CAP_HEIGHT, RATE_BITS, NUM_QUERIES, ARITY_BITS = 64, 4, 3, 28, 4   # standard_recursion_config


def expected(oc, proof, dg, cap):
    code = oc.verify(proof, dg, cap)[0]
    return 0 if code == 0 else code + 10


def flipped(proof, *words):
    q = proof.copy()
    for w in words:
        q[w] ^= np.uint64(1)
    return q


class Layout:
    """Word offsets of a flat proof from p25_circuit_info and the layout comment in include/p25.h.  The number of FRI
    layers (arity 16 each) is the one whose layout has the circuit's proof_words."""

    def __init__(self, c):
        i = c.info
        db, W, R = int(i.degree_bits), int(i.num_wires), int(i.num_routed_wires)
        NC, NP, Q = int(i.num_challenges), int(i.num_partial_products), int(i.quotient_degree_factor)
        ncs, npi = int(i.num_constants_sigmas), int(i.num_public_inputs)
        self.lde_bits = db + RATE_BITS
        self.widths = [ncs, W, NC * (1 + NP), NC * Q]
        o = 0
        for name, n in (("wires_cap", CAP_WORDS), ("zs_cap", CAP_WORDS), ("quotient_cap", CAP_WORDS),
                        ("constants", 2 * (ncs - R)), ("sigmas", 2 * R), ("wires", 2 * W), ("zs", 2 * NC),
                        ("zs_next", 2 * NC), ("pps", 2 * NC * NP), ("quotient", 2 * NC * Q)):
            setattr(self, name, o)
            o += n
        self.openings_end = self.fri_caps = o
        for k in range(9):
            if db - ARITY_BITS * k < 0 or self.lde_bits - ARITY_BITS * k < CAP_HEIGHT:
                break
            self.n_layers = k
            depth0 = self.lde_bits - CAP_HEIGHT
            # inside a query round: (leaf offset, leaf words, sibling offset, sibling words) per tree
            self.trees, q = [], 0
            for w in self.widths:
                self.trees.append((q, w, q + w, 4 * depth0))
                q += w + 4 * depth0
            for l in range(k):
                depth = self.lde_bits - ARITY_BITS * (l + 1) - CAP_HEIGHT
                self.trees.append((q, 2 << ARITY_BITS, q + (2 << ARITY_BITS), 4 * depth))
                q += (2 << ARITY_BITS) + 4 * depth
            self.query_stride = q
            self.queries = o + k * CAP_WORDS
            self.final_poly = self.queries + NUM_QUERIES * q
            self.final_poly_len = 1 << (db - ARITY_BITS * k)
            self.pow_witness = self.final_poly + 2 * self.final_poly_len
            self.public_inputs = self.pow_witness + 1
            self.total = self.public_inputs + npi
            if self.total == int(i.proof_words):
                return
        raise AssertionError("no FRI shape gives the circuit's proof_words")

    def leaf(self, query, tree, word=0):
        return self.queries + query * self.query_stride + self.trees[tree][0] + word

    def sibling(self, query, tree, word=0):
        assert self.trees[tree][3] > 0
        return self.queries + query * self.query_stride + self.trees[tree][2] + word


def reference_gates_inputs(oracle, x, y, z):
    """Inputs of gadget 14: the operands and, natively, what the reference's four gates compute."""
    spread = lambda v: sum(((v >> i) & 1) << (2 * i) for i in range(32))   # noqa: E731
    m, xi, yi = x * y % P, spread(x), spread(y)
    s = x * y + z
    lo, hi = s & 0xFFFFFFFF, s >> 32
    h = oracle.poseidon2_permute(np.array([m, xi, yi, 0, x, lo, hi, x, 0, 0, 0, 0], dtype=np.uint64))[0]
    return [x, y, z, m, xi, yi, 0, x, lo, hi] + [int(v) for v in h[:4]]
