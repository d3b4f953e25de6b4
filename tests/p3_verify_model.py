"""A plain-Python statement of the reference's plonky3 verifier, on the flat proof words of tests/p3json.py.

Written from the reference's sources in Python integers, statement by statement, so that it returns the code of the FIRST
check the sequential verifier fails:
    src/p3/verifier.rs          __p3_verify_proof__ :100-240, p3_verify_opening_proof :242-355,
                                p3_verify_shape_and_sample_challenges :357-388, p3_verify_challenges :390-417,
                                p3_verify_query :419-519
    src/p3/commit.rs            hash_iter_slices :23-46, compress :48-60, verify_batch :62-129
    src/p3/challenger.rs        the duplex challenger :70-169
    src/p3/serde/two_adic.rs    domains, selectors_at_point, zp_at_point, split_domains
The permutation is the oracle's (oracle.poseidon2_permute).  Nothing here is shared with the library's verifier
(plonky2.5_amd/csrc/p3_verify_lanes.h): it is the expected value of that code's tests, and is itself pinned to the oracle's
witness of the reference's verifier circuit (tests/test_p3_verify_model_cpu.py)."""
import numpy as np

P = 0xFFFFFFFF00000001
OK, MALFORMED, POW, INPUT_MERKLE, FRI_MERKLE, FINAL_POLY, CONSTRAINTS = 0, 30, 31, 32, 33, 34, 35
GENERATOR = 7
ROOT_2_32 = 1753635133440165772


def root_of_unity(bits):
    return pow(ROOT_2_32, 1 << (32 - bits), P)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ---- F_p[X] / (X^2 - 7), elements as (a, b) ----
def e(a):
    return (a % P, 0)


def e_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def e_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def e_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def e_inv(x):
    n = (x[0] * x[0] - 7 * x[1] * x[1]) % P
    if n == 0:
        raise ZeroDivisionError
    ni = pow(n, P - 2, P)
    return (x[0] * ni % P, (P - x[1]) * ni % P)


def e_pow2(x, k):
    for _ in range(k):
        x = e_mul(x, x)
    return x


class Shape:
    """The shape of a proof: a P3Config (binding.P3Config or anything with its fields) and the AIR's width."""

    def __init__(self, cfg):
        self.k = int(cfg.log_trace_height)
        self.B = int(cfg.log_blowup)
        self.L = self.k + self.B
        self.lqd = int(cfg.log_quotient_degree)
        self.Q = 1 << self.lqd
        self.W = int(cfg.trace_width)
        self.queries = int(cfg.num_queries)
        self.pow_bits = int(cfg.proof_of_work_bits)
        assert int(cfg.opening_matrix_log_max_height) == self.L and int(cfg.degree_bits) == self.k

    # word offsets, in `add_virtual_to` order (tests/p3json.py)
    @property
    def o_trace_local(self): return 8
    @property
    def o_trace_next(self): return 8 + 2 * self.W
    @property
    def o_chunks(self): return 8 + 4 * self.W
    @property
    def o_fri_roots(self): return 8 + 4 * self.W + 4 * self.Q
    @property
    def o_query_proofs(self): return self.o_fri_roots + 4 * self.k
    @property
    def query_proof_words(self): return sum(2 + 4 * (self.L - r - 1) for r in range(self.k))
    @property
    def o_final_poly(self): return self.o_query_proofs + self.queries * self.query_proof_words
    @property
    def o_pow_witness(self): return self.o_final_poly + 2
    @property
    def o_query_openings(self): return self.o_pow_witness + 1
    @property
    def query_opening_words(self): return self.W + 4 * self.L + 2 * self.Q + 4 * self.L
    @property
    def num_inputs(self): return self.o_query_openings + self.queries * self.query_opening_words

    def step(self, q, r):
        """Offset of commit_phase_openings[r] of query q: sibling_value (2 words), then its path."""
        return self.o_query_proofs + q * self.query_proof_words + sum(2 + 4 * (self.L - i - 1) for i in range(r))

    def opening(self, q, batch):
        """Offset of query q's opened row of batch 0 (trace) / 1 (quotient chunks); the path follows the row."""
        o = self.o_query_openings + q * self.query_opening_words
        return o if batch == 0 else o + self.W + 4 * self.L


class Challenger:
    """challenger.rs:70-169."""

    def __init__(self, permute):
        self.permute, self.state, self.inb, self.outb = permute, [0] * 12, [], []

    def duplexing(self):
        for i, v in enumerate(self.inb):
            self.state[i] = v
        self.inb = []
        self.state = self.permute(self.state)
        self.outb = list(self.state)

    def observe(self, values):
        for v in values:
            self.outb = []
            self.inb.append(v)
            if len(self.inb) == 12:
                self.duplexing()

    def sample(self):
        if self.inb or not self.outb:
            self.duplexing()
        return self.outb.pop()

    def sample_ext(self):
        a = self.sample()
        b = self.sample()
        return (a, b)

    def sample_bits(self, bits):
        return self.sample() & ((1 << bits) - 1)


def _eval_air(air, local, nxt, sels, alpha):
    """air.rs VerifierConstraintFolder over the DAG of a binding.Air: the constraints folded with alpha in order."""
    v = []
    for op, a, b, value in air.nodes:
        if op == 0:
            v.append(local[a])
        elif op == 1:
            v.append(nxt[a])
        elif op == 2:
            v.append(e(value))
        elif op == 3:
            v.append(e_add(v[a], v[b]))
        elif op == 4:
            v.append(e_sub(v[a], v[b]))
        else:
            v.append(e_mul(v[a], v[b]))
    acc = e(0)
    for node, when in air.constraints:
        c = v[node] if when == 0 else e_mul(sels[when], v[node])
        acc = e_add(e_mul(acc, alpha), c)
    return acc


def verify(oracle, air, cfg, words):
    """-> OK or the code of the first failed check.  air: binding.Air; cfg: the proof's P3Config; words: the flat proof."""
    s = Shape(cfg)
    w = [int(x) for x in np.asarray(words, dtype=np.uint64)]
    assert len(w) == s.num_inputs and air.width == s.W
    if any(x >= P for x in w):
        return MALFORMED

    def permute(state):
        return [int(x) for x in oracle.poseidon2_permute(np.array(state, dtype=np.uint64))[0]]

    def ext(o):
        return (w[o], w[o + 1])

    def hash_slices(flat):                                   # commit.rs:23-46, RATE = 4
        state = [0] * 12
        for i in range(0, len(flat), 4):
            chunk = flat[i:i + 4]
            state[:len(chunk)] = chunk
            state = permute(state)
        return state[:4]

    def verify_batch(commit, index, flat_row, path):         # commit.rs:62-129, every matrix of the batch has one height
        root = hash_slices(flat_row)
        for sib in path:
            left, right = (sib, root) if index & 1 else (root, sib)
            root = permute(left + right + [0] * 4)[:4]
            index >>= 1
        return root == commit

    def digests(o, n):
        return [w[o + 4 * i:o + 4 * i + 4] for i in range(n)]

    trace_root, quot_root = w[0:4], w[4:8]
    # verifier.rs:135-139
    ch = Challenger(permute)
    ch.observe(trace_root)
    alpha = ch.sample_ext()
    ch.observe(quot_root)
    zeta = ch.sample_ext()
    g = root_of_unity(s.k)
    zeta_next = e_mul(zeta, e(g))
    # p3_verify_opening_proof :258-262
    fri_alpha = ch.sample_ext()
    fri_roots = digests(s.o_fri_roots, s.k)
    betas = []
    for r in range(s.k):
        ch.observe(fri_roots[r])
        betas.append(ch.sample_ext())
    ch.observe([w[s.o_pow_witness]])                         # p3_check_witness :376
    if ch.sample_bits(s.pow_bits) != 0:
        return POW
    log_max_height = s.k + s.B
    indices = [ch.sample_bits(log_max_height) for _ in range(s.queries)]

    # :266-344: per query, the two input batches and the reduced openings by log_height
    trace_local = [ext(s.o_trace_local + 2 * c) for c in range(s.W)]
    trace_next = [ext(s.o_trace_next + 2 * c) for c in range(s.W)]
    chunks = [[ext(s.o_chunks + 4 * c), ext(s.o_chunks + 4 * c + 2)] for c in range(s.Q)]
    reduced = []
    for q, index in enumerate(indices):
        ro, alpha_pow = {}, {}
        o = s.opening(q, 0)
        row_t = w[o:o + s.W]
        if not verify_batch(trace_root, index, row_t, digests(o + s.W, s.L)):
            return INPUT_MERKLE
        o = s.opening(q, 1)
        rows_q = [w[o + 2 * c:o + 2 * c + 2] for c in range(s.Q)]
        if not verify_batch(quot_root, index, [x for row in rows_q for x in row], digests(o + 2 * s.Q, s.L)):
            return INPUT_MERKLE
        # every domain has 2^k points (the trace domain; each chunk domain after split_domains)
        mats = [(row_t, [(zeta, trace_local), (zeta_next, trace_next)])]
        mats += [(rows_q[c], [(zeta, chunks[c])]) for c in range(s.Q)]
        bad_point = False
        for opened, points in mats:
            log_height = s.k + s.B
            rev = bitrev(index >> (log_max_height - log_height), log_height)
            x = GENERATOR * pow(root_of_unity(log_height), rev, P) % P
            for z, ps_at_z in points:
                for p_at_x, p_at_z in zip(opened, ps_at_z):
                    try:
                        quotient = e_mul(e_sub(e(p_at_x), p_at_z), e_inv(e_sub(e(x), z)))
                    except ZeroDivisionError:
                        bad_point, quotient = True, e(0)
                    ap = alpha_pow.get(log_height, e(1))
                    ro[log_height] = e_add(ro.get(log_height, e(0)), e_mul(ap, quotient))
                    alpha_pow[log_height] = e_mul(ap, fri_alpha)
        reduced.append((ro, bad_point))

    # p3_verify_challenges :390-417 with p3_verify_query :419-519
    final_poly = ext(s.o_final_poly)
    for q, index in enumerate(indices):
        ro, bad_point = reduced[q]
        if bad_point:       # a zero denominator counts as this query's final-polynomial failure, ahead of its FRI rounds (include/p25.h)
            return FINAL_POLY
        folded = e(0)
        x = pow(root_of_unity(log_max_height), bitrev(index, log_max_height), P)
        for r in range(s.k):
            log_folded_height = log_max_height - 1 - r
            folded = e_add(ro.get(log_folded_height + 1, e(0)), folded)
            index_sibling, index_pair = index ^ 1, index >> 1
            o = s.step(q, r)
            evals = [folded, folded]
            evals[index_sibling % 2] = ext(o)
            leaf = [evals[0][0], evals[0][1], evals[1][0], evals[1][1]]
            if not verify_batch(fri_roots[r], index_pair, leaf, digests(o + 2, log_folded_height)):
                return FRI_MERKLE
            xs = [x, x]
            xs[index_sibling % 2] = x * (P - 1) % P          # the two-adic generator of order 2
            num = e_mul(e_sub(evals[1], evals[0]), e_sub(betas[r], e(xs[0])))
            folded = e_add(evals[0], e_mul(num, e(pow((xs[1] - xs[0]) % P, P - 2, P))))
            index = index_pair
            x = x * x % P
        if folded != final_poly:
            return FINAL_POLY

    # :169-239: the quotient identity at zeta
    n = 1 << s.k
    w_q = root_of_unity(s.k + s.lqd)
    shifts = [GENERATOR * pow(w_q, c, P) % P for c in range(s.Q)]       # split_domains of the disjoint coset 7 H_{n Q}

    def zp(shift, point):                                   # zp_at_point of shift * H_n
        return e_sub(e_pow2(e_mul(point, e(pow(shift, P - 2, P))), s.k), e(1))

    zps = []
    for i in range(s.Q):
        acc = e(1)
        for j in range(s.Q):
            if j != i:
                first = (pow(shifts[i] * pow(shifts[j], P - 2, P) % P, n, P) - 1) % P
                acc = e_mul(acc, e_mul(zp(shifts[j], zeta), e(pow(first, P - 2, P))))
        zps.append(acc)
    quotient = e(0)
    for c in range(s.Q):
        for e_i, part in enumerate(chunks[c]):
            monomial = (1, 0) if e_i == 0 else (0, 1)
            quotient = e_add(quotient, e_mul(zps[c], e_mul(monomial, part)))
    z_h = e_sub(e_pow2(zeta, s.k), e(1))
    g_inv = pow(g, P - 2, P)
    try:
        sels = [None, e_mul(z_h, e_inv(e_sub(zeta, e(1)))), e_mul(z_h, e_inv(e_sub(zeta, e(g_inv)))), e_sub(zeta, e(g_inv))]
        inv_zeroifier = e_inv(z_h)
    except ZeroDivisionError:
        return CONSTRAINTS
    folded_constraints = _eval_air(air, trace_local, trace_next, sels, alpha)
    if e_mul(folded_constraints, inv_zeroifier) != quotient:
        return CONSTRAINTS
    return OK
