"""A plain-Python plonky3 PROVER for the AIR form of include/p25.h: what p25_p3_prove_air_ax must write, word for word.

Written from the interface's description (include/p25.h: the stages under "The inner plonky3 STARK on the device", PUBLIC
VALUES, PERIODIC / PREPROCESSED / AUXILIARY COLUMNS) and from the verifier models tests/p3_*_model.py, which fix every
formula a proof has to satisfy -- not from the library's prover.  Python integers throughout and NO transform: a column is
the polynomial of degree < n through its values, evaluated point by point in barycentric form (O(n) a point), so nothing
here shares code or an algorithm with ntt().  The permutation is the oracle's.

    trace        column c is the polynomial through (w_n^r, trace[r][c]); leaf i of its commitment holds the columns at
                 x_i = 7 w_N^bitrev(i), N = n 2^log_blowup; Poseidon2 MMCS (sponge of rate 4 on a leaf, 2-to-1 compression)
    transcript   trace root | preprocessed root | public values; challenges; aux root; alpha; quotient root; zeta; the FRI
                 alpha; per round: the layer's root, beta; the proof-of-work witness; the query indices
    quotient     q = C / Z_H on the quotient coset 7 H_{n Q} (Q = 2^log_quotient_degree, log2_ceil(degree - 1), degree >= 2),
                 C the constraints folded with alpha under the selectors the verifier uses.  Chunk c is q on the coset
                 7 w_{nQ}^c H_n, as the polynomial of degree < n through those n values, split into its two components;
                 committed as ONE batch whose leaf i holds chunk 0's two components, chunk 1's, ... at x_i
    openings     every column of every matrix at zeta (and zeta w_n for trace, preprocessed, auxiliary)
    FRI          layer 0 is the reduced opening at every x_i (the verifier's sum, in its order); leaf j of a layer's
                 commitment holds entries 2 j and 2 j + 1; the fold is the verifier's; log_n rounds; final_poly is entry 0 of
                 the last layer (2^log_blowup entries, all equal for an honest proof)
    PoW          the smallest witness >= pow_start whose sample has pow_bits zero bits
    queries      per index the rows and paths of the input batches, per round the sibling entry and the pair's path

prove(..., fault=...) applies ONE fault at the stage named (tests/p3_forged_cases.py has the table) and finishes the proof
honestly from the faulted data; the model has none of the self-checks a real prover would trip on."""
import numpy as np

from p3_verify_model import (P, GENERATOR, Challenger, root_of_unity, bitrev, e, e_add, e_sub, e_mul, e_inv, e_pow2)
from p3_aux_model import Shape, eval_nodes, running_sums, _permute_fn
from p3_periodic_model import periodic_at

def inv(a):
    return pow(a, P - 2, P)


# ---- the shape -------------------------------------------------------------------------------------------------------
def degree(air):
    """The AIR's constraint degree, selector included: LOCAL / NEXT / PERIODIC / PREP_* / AUX_* count 1, CONST / PUBLIC /
    CHALLENGE 0, MUL adds, ADD / SUB take the greater; a first-row, last-row or transition selector adds 1."""
    d = []
    for op, a, b, _v in air.nodes:
        d.append(1 if op in (0, 1, 7, 8, 9, 11, 12) else 0 if op in (2, 6, 10) else d[a] + d[b] if op == 5 else max(d[a], d[b]))
    return max(d[node] + (1 if when else 0) for node, when in air.constraints)


def log_quotient_degree(air):
    return (max(degree(air), 2) - 2).bit_length()            # log2_ceil(degree - 1)


class Config:
    """The fields of p25_p3_config, derived here."""

    def __init__(self, air, log_n, log_blowup, num_queries, pow_bits):
        self.log_blowup, self.num_queries, self.proof_of_work_bits = log_blowup, num_queries, pow_bits
        self.log_quotient_degree, self.log_trace_height, self.trace_width = log_quotient_degree(air), log_n, air.width
        self.opening_matrix_log_max_height, self.degree_bits = log_n + log_blowup, log_n
        self.quotient_opened_len = 2                         # per chunk: its two components

    FIELDS = ("log_blowup", "num_queries", "proof_of_work_bits", "log_quotient_degree", "log_trace_height", "trace_width",
              "opening_matrix_log_max_height", "quotient_opened_len", "degree_bits")

    def same_as(self, cfg):
        return all(int(getattr(cfg, f)) == getattr(self, f) for f in self.FIELDS)


# ---- polynomials through values, point by point ------------------------------------------------------------------------
class Coset:
    """Polynomials of degree < n = 2^k given by their values at shift w_n^r: evaluation at a point, barycentric."""

    def __init__(self, k, shift=1):
        self.n = 1 << k
        self.k = k
        w = root_of_unity(k)
        self.dom = [pow(w, r, P) for r in range(self.n)]
        self.shift_inv = inv(shift)
        self.n_inv = inv(self.n)
        self._base, self._ext = {}, {}

    def weights(self, x):
        """-> (r, None) if x is the domain's point r, else (None, [l_r(x)])."""
        if x not in self._base:
            y = x * self.shift_inv % P
            if y in self.dom:
                self._base[x] = (self.dom.index(y), None)
            else:
                zh = (pow(y, self.n, P) - 1) * self.n_inv % P
                self._base[x] = (None, [zh * d % P * inv((y - d) % P) % P for d in self.dom])
        return self._base[x]

    def at(self, vals, x):
        r, wts = self.weights(x)
        return vals[r] if wts is None else sum(v * l for v, l in zip(vals, wts)) % P

    def weights_ext(self, z):
        if z not in self._ext:
            y = e_mul(z, e(self.shift_inv))
            zh = e_mul(e_sub(e_pow2(y, self.k), e(1)), e(self.n_inv))
            self._ext[z] = [e_mul(zh, e_mul(e(d), e_inv(e_sub(y, e(d))))) for d in self.dom]
        return self._ext[z]

    def at_ext(self, vals, z):
        a = b = 0
        for v, (la, lb) in zip(vals, self.weights_ext(z)):
            a += v * la
            b += v * lb
        return (a % P, b % P)


# ---- the MMCS ----------------------------------------------------------------------------------------------------------
def merkle(oracle, rows):
    """rows[i] = the words of leaf i -> the tree's levels, leaf digests first, the root's level last."""
    rows = np.array(rows, dtype=np.uint64)
    states = np.zeros((rows.shape[0], 12), dtype=np.uint64)
    for off in range(0, rows.shape[1], 4):
        m = min(4, rows.shape[1] - off)
        states[:, :m] = rows[:, off:off + m]
        states = oracle.poseidon2_permute(states)
    levels = [states[:, :4].copy()]
    while levels[-1].shape[0] > 1:
        st = np.zeros((levels[-1].shape[0] // 2, 12), dtype=np.uint64)
        st[:, 0:4], st[:, 4:8] = levels[-1][0::2], levels[-1][1::2]
        levels.append(oracle.poseidon2_permute(st)[:, :4].copy())
    return levels


def root(levels):
    return [int(v) for v in levels[-1][0]]


def path(levels, index):
    out = []
    for lv in levels[:-1]:
        out += [int(v) for v in lv[index ^ 1]]
        index >>= 1
    return out


# ---- the prover --------------------------------------------------------------------------------------------------------
class Proof:
    """words (uint64, public values last), cfg (Config), shape (p3_aux_model.Shape) and what the transcript gave:
    zeta, indices, pow_witness, challenges."""


def prove(oracle, air, trace, log_blowup=1, num_queries=3, pow_bits=4, pow_start=0, public_values=None, fault=None):
    """fault: None or one of ("row", r, c), ("aux_start", j), ("chunk", c, comp), ("opened", section, i), ("fold", r),
    ("final", comp); section: trace_local / trace_next / chunks / prep_local / prep_next / aux_local / aux_next, i a word index in
    it (negative from the end).  An unbalanced trace or one built for other public values is simply passed as `trace`."""
    kind = fault[0] if fault else None
    trace = [[int(v) for v in row] for row in np.asarray(trace, dtype=np.uint64)]
    n = len(trace)
    k = n.bit_length() - 1
    assert n == 1 << k and all(len(r) == air.width for r in trace)
    cfg = Config(air, k, log_blowup, num_queries, pow_bits)
    lqd, Q, B, L = cfg.log_quotient_degree, 1 << cfg.log_quotient_degree, log_blowup, k + log_blowup
    assert lqd <= B
    pv = [int(v) for v in public_values] if public_values is not None else []
    assert len(pv) == air.n_public
    prep = None if air.preprocessed is None else [[int(v) for v in r] for r in air.preprocessed]
    pw = len(prep[0]) if prep else 0
    aw = len(air.aux_columns)
    s = Shape(cfg, pw, aw)
    permute = _permute_fn(oracle)
    if kind == "row":
        trace[fault[1]][fault[2]] = (trace[fault[1]][fault[2]] + 1) % P

    H = Coset(k)
    g = root_of_unity(k)
    w_big = root_of_unity(L)
    xs = [GENERATOR * pow(w_big, bitrev(i, L), P) % P for i in range(1 << L)]

    def columns(rows):
        return [[r[c] for r in rows] for c in range(len(rows[0]))]

    def lde(cols):
        return [[H.at(col, x) for col in cols] for x in xs]

    # the trace, the key's commitment, the public values
    t_cols = columns(trace)
    t_lde = lde(t_cols)
    t_tree = merkle(oracle, t_lde)
    ch = Challenger(permute)
    ch.observe(root(t_tree))
    if pw:
        p_cols = columns(prep)
        p_lde = lde(p_cols)
        p_tree = merkle(oracle, p_lde)
        ch.observe(root(p_tree))
    ch.observe(pv)
    # the challenge phase
    challenges, a_cols = [], []
    if aw:
        challenges = [ch.sample_ext() for _ in range(air.n_challenges)]
        sums = running_sums(air, trace, pv, challenges)
        if kind == "aux_start":
            sums = [[e_add(v, e(1)) if j == fault[1] else v for j, v in enumerate(row)] for row in sums]
        a_cols = columns([[c for v in row for c in v] for row in sums])          # column j's components at 2 j, 2 j + 1
        a_lde = lde(a_cols)
        a_tree = merkle(oracle, a_lde)
        ch.observe(root(a_tree))
    alpha = ch.sample_ext()

    # the quotient on 7 H_{n Q}, point j = 7 w_{nQ}^j; the next row of point j is point j + Q
    nq = n * Q
    w_q = root_of_unity(k + lqd)
    qx = [GENERATOR * pow(w_q, j, P) % P for j in range(nq)]
    g_inv = inv(g)

    def on_coset(cols):
        return [[e(H.at(col, x)) for col in cols] for x in qx]
    t_q = on_coset(t_cols)
    p_q = on_coset(p_cols) if pw else None
    a_q = [[(row[2 * j][0], row[2 * j + 1][0]) for j in range(aw)] for row in on_coset(a_cols)] if aw else None
    quotient = []
    for j, x in enumerate(qx):
        j1 = (j + Q) % nq
        z_h = (pow(x, n, P) - 1) % P
        sels = [None, e(z_h * inv((x - 1) % P)), e(z_h * inv((x - g_inv) % P)), e(x - g_inv)]
        per = [periodic_at(c, k, e(x)) for c in air.periodic_columns]
        v = eval_nodes(air, t_q[j], t_q[j1], pv, per, p_q[j] if pw else None, p_q[j1] if pw else None, challenges,
                       a_q[j] if aw else None, a_q[j1] if aw else None)
        acc = e(0)
        for node, when in air.constraints:
            acc = e_add(e_mul(acc, alpha), v[node] if when == 0 else e_mul(sels[when], v[node]))
        quotient.append(e_mul(acc, e(inv(z_h))))
    cosets = [Coset(k, qx[c]) for c in range(Q)]
    c_cols = []                                              # chunk c's components at 2 c and 2 c + 1
    for c in range(Q):
        vals = [quotient[c + Q * r] for r in range(n)]
        c_cols += [[v[0] for v in vals], [v[1] for v in vals]]
    if kind == "chunk":                                      # coefficient 0 is every value's constant part
        col = c_cols[2 * fault[1] + fault[2]]
        col[:] = [(v + 1) % P for v in col]
    c_lde = [[cosets[i // 2].at(col, x) for i, col in enumerate(c_cols)] for x in xs]
    c_tree = merkle(oracle, c_lde)
    ch.observe(root(c_tree))
    zeta = ch.sample_ext()
    zeta_next = e_mul(zeta, e(g))

    # the openings
    def opened(cols, z):
        return [H.at_ext(col, z) for col in cols]
    sections = {"trace_local": opened(t_cols, zeta), "trace_next": opened(t_cols, zeta_next),
                "chunks": [cosets[i // 2].at_ext(col, zeta) for i, col in enumerate(c_cols)],
                "prep_local": opened(p_cols, zeta) if pw else [], "prep_next": opened(p_cols, zeta_next) if pw else [],
                "aux_local": opened(a_cols, zeta), "aux_next": opened(a_cols, zeta_next)}
    if kind == "opened":
        sec = sections[fault[1]]
        i = fault[2] % (2 * len(sec))
        v = list(sec[i // 2])
        v[i % 2] = (v[i % 2] + 1) % P
        sec[i // 2] = tuple(v)

    # FRI: layer 0 is the reduced opening, in the verifier's order of matrices, points and columns
    fri_alpha = ch.sample_ext()
    mats = [(t_lde, 0, air.width, [(0, sections["trace_local"]), (1, sections["trace_next"])])]
    mats += [(c_lde, 2 * c, 2, [(0, sections["chunks"][2 * c:2 * c + 2])]) for c in range(Q)]
    if pw:
        mats.append((p_lde, 0, pw, [(0, sections["prep_local"]), (1, sections["prep_next"])]))
    if aw:
        mats.append((a_lde, 0, 2 * aw, [(0, sections["aux_local"]), (1, sections["aux_next"])]))
    layer = []
    for i, x in enumerate(xs):
        dinv = [e_inv(e_sub(e(x), zeta)), e_inv(e_sub(e(x), zeta_next))]
        ro, ap = e(0), e(1)
        for rows, first, width, points in mats:
            for which, at_z in points:
                for c in range(width):
                    ro = e_add(ro, e_mul(ap, e_mul(e_sub(e(rows[i][first + c]), at_z[c]), dinv[which])))
                    ap = e_mul(ap, fri_alpha)
        layer.append(ro)
    layers, trees, betas = [], [], []
    for r in range(k):
        if kind == "fold" and r == fault[1] + 1:
            layer = [e_add(v, e(1)) for v in layer]
        layers.append(layer)
        trees.append(merkle(oracle, [list(layer[2 * j]) + list(layer[2 * j + 1]) for j in range(len(layer) // 2)]))
        ch.observe(root(trees[r]))
        beta = ch.sample_ext()
        betas.append(beta)
        w_r = root_of_unity(L - r)
        nxt = []
        for j in range(len(layer) // 2):
            x0 = pow(w_r, bitrev(2 * j, L - r), P)
            num = e_mul(e_sub(layer[2 * j + 1], layer[2 * j]), e_sub(beta, e(x0)))
            nxt.append(e_add(layer[2 * j], e_mul(num, e(inv((P - 2 * x0) % P)))))
        layer = nxt
    assert len(layer) == 1 << B
    final_poly = list(layer[0])
    if kind == "final":
        final_poly[fault[1]] = (final_poly[fault[1]] + 1) % P

    # the proof of work and the query indices
    witness = pow_start
    while True:
        c2 = Challenger(permute)
        c2.state, c2.inb, c2.outb = list(ch.state), list(ch.inb), list(ch.outb)
        c2.observe([witness])
        if c2.sample_bits(pow_bits) == 0:
            break
        witness += 1
        assert witness < P
    indices = [c2.sample_bits(L) for _ in range(num_queries)]

    # the words
    def flat(values):
        return [c for v in values for c in v]
    w = root(t_tree) + root(c_tree) + flat(sections["trace_local"]) + flat(sections["trace_next"]) + flat(sections["chunks"])
    assert len(w) == s.o_prep_local
    w += flat(sections["prep_local"]) + flat(sections["prep_next"])
    if aw:
        assert len(w) == s.o_aux_commit
        w += root(a_tree) + flat(sections["aux_local"]) + flat(sections["aux_next"])
    assert len(w) == s.o_fri_roots
    for r in range(k):
        w += root(trees[r])
    for q, index in enumerate(indices):
        for r in range(k):
            assert len(w) == s.step(q, r)
            w += list(layers[r][index ^ 1]) + path(trees[r], index >> 1)
            index >>= 1
    assert len(w) == s.o_final_poly
    w += final_poly + [witness]
    for q, index in enumerate(indices):
        assert len(w) == s.opening(q, 0)
        w += t_lde[index] + path(t_tree, index) + c_lde[index] + path(c_tree, index)
        if pw:
            w += p_lde[index] + path(p_tree, index)
        if aw:
            w += a_lde[index] + path(a_tree, index)
    assert len(w) == s.num_inputs
    out = Proof()
    out.words = np.array(w + pv, dtype=np.uint64)
    out.cfg, out.shape, out.zeta, out.indices, out.pow_witness, out.challenges = cfg, s, zeta, indices, witness, challenges
    out.prep_commit = root(p_tree) if pw else None
    return out
