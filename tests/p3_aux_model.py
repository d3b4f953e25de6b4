"""The plain-Python plonky3 verifier of tests/p3_preprocessed_model.py for AIRs with AUXILIARY COLUMNS (include/p25.h).

Written from the interface's description, not from the library's code.  What differs from that model:
    transcript   behind the public values: n_challenges extension elements are sampled in index order, then the 4 words of
                 the auxiliary commitment -- PROOF words, unlike the preprocessed commitment -- are observed, then alpha
    the words    two more insertions: aux_commit u64[4] | aux_local E[2 AW] | aux_next E[2 AW] behind prep_next, and a last
                 batch {row u64[2 AW], path H[log_n + log_blowup]} behind every query's other batches
    openings     one more (commitment, matrices, points) entry, the last: one matrix of the trace's height, 2 AW base columns,
                 points (zeta, aux_local), (zeta w_n, aux_next); its alpha powers continue where the slot stands
    the AIR      node ops 10 CHALLENGE(a), 11 AUX_LOCAL(a), 12 AUX_NEXT(a); column a at a point is o[2 a] + X o[2 a + 1]
    the keys     with nb = 2 + (PW > 0) + (AW > 0) input batches per query, the input checks of query q run in batch order
                 before any FRI step (key 2 + nb q + b): the model returns the code of the first failed check in that order
Everything else is that model's statement of src/p3/verifier.rs, returning the same codes.  Without auxiliary columns this is
that model.

The AIR is taken as data: anything with .nodes, .constraints, .width, .n_public, .periodic_columns, .preprocessed,
.n_challenges and .aux_columns (binding.Air has them)."""
import numpy as np

from p3_verify_model import (P, OK, MALFORMED, POW, INPUT_MERKLE, FRI_MERKLE, FINAL_POLY, CONSTRAINTS, GENERATOR,
                             Challenger, root_of_unity, bitrev, e, e_add, e_sub, e_mul, e_inv, e_pow2)
import p3_preprocessed_model
from p3_periodic_model import periodic_at


class Shape(p3_preprocessed_model.Shape):
    """The shape of a proof with PW preprocessed and AW auxiliary columns."""

    def __init__(self, cfg, pw, aw):
        super().__init__(cfg, pw)
        self.AW = int(aw)

    @property
    def nb(self): return 2 + (1 if self.PW else 0) + (1 if self.AW else 0)
    @property
    def o_aux_commit(self): return self.o_prep_local + 4 * self.PW
    @property
    def o_aux_local(self): return self.o_aux_commit + 4
    @property
    def o_aux_next(self): return self.o_aux_local + 4 * self.AW
    @property
    def o_fri_roots(self): return self.o_prep_local + 4 * self.PW + ((4 + 8 * self.AW) if self.AW else 0)
    @property
    def query_opening_words(self):
        return (self.W + 4 * self.L + 2 * self.Q + 4 * self.L + ((self.PW + 4 * self.L) if self.PW else 0) +
                ((2 * self.AW + 4 * self.L) if self.AW else 0))

    def opening(self, q, batch):
        """batch: 0 trace, 1 quotient, 2 preprocessed, 3 auxiliary (the last, wherever that is)."""
        o = self.o_query_openings + q * self.query_opening_words
        offs = [0, self.W + 4 * self.L, self.W + 2 * self.Q + 8 * self.L,
                self.W + 2 * self.Q + 8 * self.L + ((self.PW + 4 * self.L) if self.PW else 0)]
        return o + offs[batch]


def num_inputs_formula(cfg, pw, aw, n_public):
    """num_inputs grows by 4 + 8 AW + num_queries (2 AW + 4 (log_n + log_blowup))."""
    base = p3_preprocessed_model.num_inputs_formula(cfg, pw, n_public)
    return base + ((4 + 8 * aw + int(cfg.num_queries) * (2 * aw + 4 * (int(cfg.log_trace_height) + int(cfg.log_blowup)))) if aw else 0)


def regions(cfg, pw, aw):
    """Word ranges of what auxiliary columns add to a proof: {name: [(start, stop), ...]}."""
    s = Shape(cfg, pw, aw)
    out = {"aux_commit": [(s.o_aux_commit, s.o_aux_local)], "aux_local": [(s.o_aux_local, s.o_aux_next)],
           "aux_next": [(s.o_aux_next, s.o_fri_roots)], "row": [], "path": []}
    for q in range(s.queries):
        o = s.opening(q, 3)
        out["row"].append((o, o + 2 * aw))
        out["path"].append((o + 2 * aw, o + 2 * aw + 4 * s.L))
    return out


def eval_nodes(air, local, nxt, public_values, periodic, prep_local, prep_next, challenges, aux_local, aux_next):
    """The values of every node of the DAG in F_p^2, ops 0..12.  aux_local = None (the column builder's call): the nodes
    that depend on an auxiliary column have no value, None."""
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
        elif op == 10:
            v.append(challenges[a])
        elif op == 11:
            v.append(aux_local[a] if aux_local is not None else None)
        elif op == 12:
            v.append(aux_next[a] if aux_next is not None else None)
        elif v[a] is None or v[b] is None:
            v.append(None)
        elif op == 3:
            v.append(e_add(v[a], v[b]))
        elif op == 4:
            v.append(e_sub(v[a], v[b]))
        else:
            assert op == 5
            v.append(e_mul(v[a], v[b]))
    return v


def running_sums(air, trace, public_values, challenges):
    """The auxiliary columns from their definition: S_j(0) = 0, S_j(i + 1) = S_j(i) + num_j(i) / den_j(i) on trace row i
    (NEXT: row (i + 1) mod n) -> [n][AW] extension elements; raises ZeroDivisionError at a zero denominator."""
    n = len(trace)
    aw = len(air.aux_columns)
    rows = [[e(int(x)) for x in r] for r in trace]
    prep = None if air.preprocessed is None else [[e(int(x)) for x in r] for r in air.preprocessed]
    out, run = [], [e(0)] * aw
    for i in range(n):
        out.append(list(run))
        i1 = (i + 1) % n
        per = [e(int(c[i % len(c)])) for c in air.periodic_columns]
        v = eval_nodes(air, rows[i], rows[i1], public_values, per, prep[i] if prep else None, prep[i1] if prep else None,
                       challenges, None, None)
        run = [e_add(run[j], e_mul(v[nu], e_inv(v[de]))) for j, (nu, de) in enumerate(air.aux_columns)]
    return out


def _permute_fn(oracle):
    def permute(state):
        return [int(x) for x in oracle.poseidon2_permute(np.array(state, dtype=np.uint64))[0]]
    return permute


def challenges_of(oracle, air, words, cfg, prep_commit=None):
    """The challenges the transcript of this proof gives (for tests that restate the columns from their definition)."""
    w = [int(x) for x in np.asarray(words, dtype=np.uint64)]
    ch = Challenger(_permute_fn(oracle))
    ch.observe(w[0:4])
    if prep_commit is not None:
        ch.observe([int(x) for x in prep_commit])
    ch.observe(w[len(w) - int(air.n_public):] if air.n_public else [])
    return [ch.sample_ext() for _ in range(air.n_challenges)]


def verify(oracle, air, cfg, words, prep_commit=None):
    """-> OK or the code of the first failed check.  words: the flat proof, its air.n_public public values last.
    prep_commit: the 4 words of the verifying key's preprocessed commitment (None without preprocessed columns)."""
    pw = 0 if air.preprocessed is None else int(air.preprocessed.shape[1])
    aw = len(air.aux_columns)
    s = Shape(cfg, pw, aw)
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
    aux_root = w[s.o_aux_commit:s.o_aux_commit + 4] if aw else None
    ch = Challenger(permute)
    ch.observe(trace_root)
    if pw:
        ch.observe(prep_root)
    ch.observe(public_values)
    challenges = []
    if aw:                                                   # the challenge phase
        challenges = [ch.sample_ext() for _ in range(air.n_challenges)]
        ch.observe(aux_root)
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
    aux_local = [ext(s.o_aux_local + 2 * c) for c in range(2 * aw)]
    aux_next = [ext(s.o_aux_next + 2 * c) for c in range(2 * aw)]
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
        if pw:
            o = s.opening(q, 2)
            row_p = w[o:o + pw]
            if not verify_batch(prep_root, index, row_p, digests(o + pw, L)):
                return INPUT_MERKLE
            mats.append((row_p, [(zeta, prep_local), (zeta_next, prep_next)]))
        if aw:                                               # the last batch: against the PROOF's aux_commit
            o = s.opening(q, 3)
            row_a = w[o:o + 2 * aw]
            if not verify_batch(aux_root, index, row_a, digests(o + 2 * aw, L)):
                return INPUT_MERKLE
            mats.append((row_a, [(zeta, aux_local), (zeta_next, aux_next)]))
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
    periodic = [periodic_at(c, s.k, zeta) for c in air.periodic_columns]
    # an auxiliary column at a point: o[2 a] + X o[2 a + 1], X the extension's generator
    al = [e_add(aux_local[2 * c], e_mul((0, 1), aux_local[2 * c + 1])) for c in range(aw)]
    an = [e_add(aux_next[2 * c], e_mul((0, 1), aux_next[2 * c + 1])) for c in range(aw)]
    v = eval_nodes(air, trace_local, trace_next, public_values, periodic, prep_local, prep_next, challenges, al, an)
    acc = e(0)
    for node, when in air.constraints:
        c = v[node] if when == 0 else e_mul(sels[when], v[node])
        acc = e_add(e_mul(acc, alpha), c)
    if e_mul(acc, inv_zeroifier) != quotient:
        return CONSTRAINTS
    return OK
