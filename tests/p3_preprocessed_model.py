"""The plain-Python plonky3 verifier of tests/p3_periodic_model.py for AIRs with PREPROCESSED COLUMNS (include/p25.h).

Written from the interface's description, not from the library's code.  What differs from that model:
    the key      the 4 words of the preprocessed commitment are an ARGUMENT (verifying-key data); the model never recomputes
                 them from the columns -- it reaches them through every query's Merkle path only
    transcript   the commitment is observed directly after the trace commitment, before the public values and alpha
    the words    `add_virtual_to` order with two insertions: prep_local E[PW] | prep_next E[PW] behind the chunk openings, and
                 a third batch {row u64[PW], path H[log_n + log_blowup]} behind every query's quotient batch
    openings     a third (commitment, matrices, points) entry: one matrix of the trace's height with the points
                 (zeta, prep_local), (zeta w_n, prep_next); its alpha powers continue behind the quotient chunks'
    the AIR      node ops 8 PREP_LOCAL(a) / 9 PREP_NEXT(a) read the two opened rows
Everything else is that model's statement of src/p3/verifier.rs, returning the same codes.  Without columns (PW = 0, no
commitment) this is that model.

model_commit() states the commitment itself -- Lagrange interpolation over <w_n>, evaluated point by point on
7 H_{n 2^log_blowup}, hashed with the oracle's permutation -- sharing no transform, LDE or tree code with the library."""
import numpy as np

from p3_verify_model import (P, OK, MALFORMED, POW, INPUT_MERKLE, FRI_MERKLE, FINAL_POLY, CONSTRAINTS, GENERATOR,
                             Challenger, root_of_unity, bitrev, e, e_add, e_sub, e_mul, e_inv, e_pow2)
import p3_verify_model
from p3_periodic_model import periodic_at


class Shape(p3_verify_model.Shape):
    """The shape of a proof with PW preprocessed columns: the two insertions move what stands behind them."""

    def __init__(self, cfg, pw):
        super().__init__(cfg)
        self.PW = int(pw)

    @property
    def o_prep_local(self): return 8 + 4 * self.W + 4 * self.Q
    @property
    def o_prep_next(self): return self.o_prep_local + 2 * self.PW
    @property
    def o_fri_roots(self): return self.o_prep_local + 4 * self.PW
    @property
    def query_opening_words(self):
        return self.W + 4 * self.L + 2 * self.Q + 4 * self.L + ((self.PW + 4 * self.L) if self.PW else 0)

    def opening(self, q, batch):
        o = self.o_query_openings + q * self.query_opening_words
        return o + [0, self.W + 4 * self.L, self.W + 2 * self.Q + 8 * self.L][batch]


def num_inputs_formula(cfg, pw, n_public):
    """The issue's formula: the words p25_p3_config describes + 4 PW + num_queries (PW + 4 (log_n + log_blowup)) + n_public."""
    base = p3_verify_model.Shape(cfg).num_inputs
    extra = 4 * pw + int(cfg.num_queries) * (pw + 4 * (int(cfg.log_trace_height) + int(cfg.log_blowup))) if pw else 0
    return base + extra + n_public


def regions(cfg, pw):
    """Word ranges of what preprocessed columns add to a proof: {name: [(start, stop), ...]}."""
    s = Shape(cfg, pw)
    out = {"prep_local": [(s.o_prep_local, s.o_prep_next)], "prep_next": [(s.o_prep_next, s.o_fri_roots)], "row": [], "path": []}
    for q in range(s.queries):
        o = s.opening(q, 2)
        out["row"].append((o, o + pw))
        out["path"].append((o + pw, o + pw + 4 * s.L))
    return out


def eval_air(air, local, nxt, public_values, periodic, prep_local, prep_next, sels, alpha):
    """air.rs VerifierConstraintFolder over the DAG of a binding.Air, ops 0..9."""
    v = []
    for op, a, b, value in air.nodes:
        if op == 0:
            v.append(local[a])
        elif op == 1:
            v.append(nxt[a])
        elif op == 2:
            v.append(e(value))
        elif op == 6:
            v.append(e(public_values[a]))
        elif op == 7:
            v.append(periodic[a])
        elif op == 8:
            v.append(prep_local[a])
        elif op == 9:
            v.append(prep_next[a])
        elif op == 3:
            v.append(e_add(v[a], v[b]))
        elif op == 4:
            v.append(e_sub(v[a], v[b]))
        else:
            assert op == 5
            v.append(e_mul(v[a], v[b]))
    acc = e(0)
    for node, when in air.constraints:
        c = v[node] if when == 0 else e_mul(sels[when], v[node])
        acc = e_add(e_mul(acc, alpha), c)
    return acc


def _permute_fn(oracle):
    def permute(state):
        return [int(x) for x in oracle.poseidon2_permute(np.array(state, dtype=np.uint64))[0]]
    return permute


def model_commit(oracle, prep, log_blowup):
    """The commitment of the matrix prep[2^log_n][PW], from its definition: column c is the polynomial of degree < n through
    (w_n^r, prep[r][c]); leaf i holds the PW values at 7 w_N^bitrev(i), N = n 2^log_blowup; Poseidon2 MMCS above them."""
    prep = np.asarray(prep, dtype=np.uint64)
    n, pw = prep.shape
    k = n.bit_length() - 1
    L = k + log_blowup
    w_n, w_big = root_of_unity(k), root_of_unity(L)
    n_inv = pow(n, P - 2, P)
    cols = [[int(v) for v in prep[:, c]] for c in range(pw)]
    dom = [pow(w_n, r, P) for r in range(n)]
    permute_many = oracle.poseidon2_permute
    leaves = []
    for i in range(n << log_blowup):
        x = GENERATOR * pow(w_big, bitrev(i, L), P) % P
        # barycentric form over <w_n>: f(x) = (x^n - 1) / n  sum_r f(w^r) w^r / (x - w^r); x lies off the domain
        zh = (pow(x, n, P) - 1) * n_inv % P
        wts = [dom[r] * pow((x - dom[r]) % P, P - 2, P) % P for r in range(n)]
        leaves.append([zh * (sum(col[r] * wts[r] for r in range(n)) % P) % P for col in cols])
    states = np.zeros((len(leaves), 12), dtype=np.uint64)
    for off in range(0, pw, 4):
        m = min(4, pw - off)
        states[:, :m] = np.array([row[off:off + m] for row in leaves], dtype=np.uint64)
        states = permute_many(states)
    level = states[:, :4].copy()
    while level.shape[0] > 1:
        st = np.zeros((level.shape[0] // 2, 12), dtype=np.uint64)
        st[:, 0:4], st[:, 4:8] = level[0::2], level[1::2]
        level = permute_many(st)[:, :4].copy()
    return [int(v) for v in level[0]]


def verify(oracle, air, cfg, words, prep_commit, pw=None, columns=None):
    """-> OK or the code of the first failed check.  words: the flat proof, its air.n_public public values last.
    prep_commit: the 4 words of the verifying key's preprocessed commitment (None with pw = 0).
    pw: the preprocessed width (default: the AIR's); columns: the periodic columns (default: the AIR's own)."""
    if pw is None:
        pw = 0 if air.preprocessed is None else int(air.preprocessed.shape[1])
    columns = air.periodic_columns if columns is None else columns
    s = Shape(cfg, pw)
    m = int(air.n_public)
    w = [int(x) for x in np.asarray(words, dtype=np.uint64)]
    assert len(w) == s.num_inputs + m and air.width == s.W
    if any(x >= P for x in w):
        return MALFORMED
    public_values = w[s.num_inputs:]
    permute = _permute_fn(oracle)

    def ext(o):
        return (w[o], w[o + 1])

    def hash_slices(flat):
        state = [0] * 12
        for i in range(0, len(flat), 4):
            chunk = flat[i:i + 4]
            state[:len(chunk)] = chunk
            state = permute(state)
        return state[:4]

    def verify_batch(commit, index, flat_row, path):
        root = hash_slices(flat_row)
        for sib in path:
            left, right = (sib, root) if index & 1 else (root, sib)
            root = permute(left + right + [0] * 4)[:4]
            index >>= 1
        return root == commit

    def digests(o, n):
        return [w[o + 4 * i:o + 4 * i + 4] for i in range(n)]

    trace_root, quot_root = w[0:4], w[4:8]
    prep_root = [int(x) for x in prep_commit] if pw else None
    ch = Challenger(permute)
    ch.observe(trace_root)
    if pw:
        ch.observe(prep_root)                                # the extra observe: verifying-key data, not proof words
    ch.observe(public_values)
    alpha = ch.sample_ext()
    ch.observe(quot_root)
    zeta = ch.sample_ext()
    g = root_of_unity(s.k)
    zeta_next = e_mul(zeta, e(g))
    fri_alpha = ch.sample_ext()
    fri_roots = digests(s.o_fri_roots, s.k)
    betas = []
    for r in range(s.k):
        ch.observe(fri_roots[r])
        betas.append(ch.sample_ext())
    ch.observe([w[s.o_pow_witness]])
    if ch.sample_bits(s.pow_bits) != 0:
        return POW
    L = s.k + s.B
    indices = [ch.sample_bits(L) for _ in range(s.queries)]

    trace_local = [ext(s.o_trace_local + 2 * c) for c in range(s.W)]
    trace_next = [ext(s.o_trace_next + 2 * c) for c in range(s.W)]
    chunks = [[ext(s.o_chunks + 4 * c), ext(s.o_chunks + 4 * c + 2)] for c in range(s.Q)]
    prep_local = [ext(s.o_prep_local + 2 * c) for c in range(pw)]
    prep_next = [ext(s.o_prep_next + 2 * c) for c in range(pw)]
    reduced = []
    for q, index in enumerate(indices):
        o = s.opening(q, 0)
        row_t = w[o:o + s.W]
        if not verify_batch(trace_root, index, row_t, digests(o + s.W, L)):
            return INPUT_MERKLE
        o = s.opening(q, 1)
        rows_q = [w[o + 2 * c:o + 2 * c + 2] for c in range(s.Q)]
        if not verify_batch(quot_root, index, [x for row in rows_q for x in row], digests(o + 2 * s.Q, L)):
            return INPUT_MERKLE
        x = GENERATOR * pow(root_of_unity(L), bitrev(index, L), P) % P
        mats = [(row_t, [(zeta, trace_local), (zeta_next, trace_next)])]
        mats += [(rows_q[c], [(zeta, chunks[c])]) for c in range(s.Q)]
        if pw:                                               # the third batch
            o = s.opening(q, 2)
            row_p = w[o:o + pw]
            if not verify_batch(prep_root, index, row_p, digests(o + pw, L)):
                return INPUT_MERKLE
            mats.append((row_p, [(zeta, prep_local), (zeta_next, prep_next)]))
        # every matrix has the height of the LDE domain: one reduced opening per query, one run of alpha powers
        ro, ap, bad_point = e(0), e(1), False
        for opened, points in mats:
            for z, ps_at_z in points:
                for p_at_x, p_at_z in zip(opened, ps_at_z):
                    try:
                        quotient = e_mul(e_sub(e(p_at_x), p_at_z), e_inv(e_sub(e(x), z)))
                    except ZeroDivisionError:
                        bad_point, quotient = True, e(0)
                    ro = e_add(ro, e_mul(ap, quotient))
                    ap = e_mul(ap, fri_alpha)
        reduced.append((ro, bad_point))

    final_poly = ext(s.o_final_poly)
    for q, index in enumerate(indices):
        ro, bad_point = reduced[q]
        if bad_point:
            return FINAL_POLY
        folded = e(0)
        x = pow(root_of_unity(L), bitrev(index, L), P)
        for r in range(s.k):
            log_folded_height = L - 1 - r
            if r == 0:
                folded = e_add(ro, folded)
            index_sibling, index_pair = index ^ 1, index >> 1
            o = s.step(q, r)
            evals = [folded, folded]
            evals[index_sibling % 2] = ext(o)
            leaf = [evals[0][0], evals[0][1], evals[1][0], evals[1][1]]
            if not verify_batch(fri_roots[r], index_pair, leaf, digests(o + 2, log_folded_height)):
                return FRI_MERKLE
            xs = [x, x]
            xs[index_sibling % 2] = x * (P - 1) % P
            num = e_mul(e_sub(evals[1], evals[0]), e_sub(betas[r], e(xs[0])))
            folded = e_add(evals[0], e_mul(num, e(pow((xs[1] - xs[0]) % P, P - 2, P))))
            index = index_pair
            x = x * x % P
        if folded != final_poly:
            return FINAL_POLY

    n = 1 << s.k
    w_q = root_of_unity(s.k + s.lqd)
    shifts = [GENERATOR * pow(w_q, c, P) % P for c in range(s.Q)]

    def zp(shift, point):
        return e_sub(e_pow2(e_mul(point, e(pow(shift, P - 2, P))), s.k), e(1))

    quotient = e(0)
    for i in range(s.Q):
        acc = e(1)
        for j in range(s.Q):
            if j != i:
                first = (pow(shifts[i] * pow(shifts[j], P - 2, P) % P, n, P) - 1) % P
                acc = e_mul(acc, e_mul(zp(shifts[j], zeta), e(pow(first, P - 2, P))))
        quotient = e_add(quotient, e_mul(acc, e_add(chunks[i][0], e_mul((0, 1), chunks[i][1]))))
    z_h = e_sub(e_pow2(zeta, s.k), e(1))
    g_inv = pow(g, P - 2, P)
    try:
        sels = [None, e_mul(z_h, e_inv(e_sub(zeta, e(1)))), e_mul(z_h, e_inv(e_sub(zeta, e(g_inv)))), e_sub(zeta, e(g_inv))]
        inv_zeroifier = e_inv(z_h)
    except ZeroDivisionError:
        return CONSTRAINTS
    periodic = [periodic_at(c, s.k, zeta) for c in columns]
    folded_constraints = eval_air(air, trace_local, trace_next, public_values, periodic, prep_local, prep_next, sels, alpha)
    if e_mul(folded_constraints, inv_zeroifier) != quotient:
        return CONSTRAINTS
    return OK
