"""The plain-Python plonky3 verifier of tests/p3_public_values_model.py for AIRs with PERIODIC COLUMNS (include/p25.h).

One thing differs from that model, and it is stated here from the interface's description, not from the library's code:
    the AIR   node op 7 PERIODIC(a) is periodic column a at zeta: c(zeta) = q(zeta^(n/P)), q the interpolant of the
              column's P values over <w_P>, w_P = w_n^(n/P).  It is evaluated here in LAGRANGE form -- with y = zeta^(n/P),
              c(zeta) = sum_j v[j] w_P^j (y^P - 1) / (P (y - w_P^j)) -- so the model shares no inverse transform, no
              coefficient and no table with the library.
The columns are neither committed nor opened and not observed: the proof's words, the shape and the transcript are that
model's.  Everything else is its statement of src/p3/verifier.rs, in the same order, returning the same codes; the shape, the
challenger and the field helpers are imported from tests/p3_verify_model.py.  Without columns this is that model."""
import numpy as np

from p3_verify_model import (P, OK, MALFORMED, POW, INPUT_MERKLE, FRI_MERKLE, FINAL_POLY, CONSTRAINTS, GENERATOR, Shape,
                             Challenger, root_of_unity, bitrev, e, e_add, e_sub, e_mul, e_inv, e_pow2)


_at_zeta = {}   # (values, log_n, zeta) -> value: most mutations of a proof leave zeta as it was


def periodic_at(values, log_n, zeta):
    """Column `values` (period P = len(values)) of a trace of 2^log_n rows at zeta, in Lagrange form over <w_P>."""
    vals = [int(v) for v in values]
    key = (tuple(vals), log_n, zeta)
    if key not in _at_zeta:
        _at_zeta[key] = _periodic_at(vals, log_n, zeta)
    return _at_zeta[key]


def _periodic_at(vals, log_n, zeta):
    big_p = len(vals)
    k = big_p.bit_length() - 1
    assert big_p == 1 << k and 1 <= k <= log_n
    y = e_pow2(zeta, log_n - k)
    yp = e_pow2(y, k)
    if yp == e(1):
        raise ValueError("zeta^(n/P) lies in <w_P>: the Lagrange form has a pole (chance about 2^-120)")
    num = e_mul(e_sub(yp, e(1)), e(pow(big_p, P - 2, P)))
    w_p = root_of_unity(k)
    acc, wj = e(0), 1
    for v in vals:
        acc = e_add(acc, e_mul(e(v * wj % P), e_inv(e_sub(y, e(wj)))))
        wj = wj * w_p % P
    return e_mul(acc, num)


def eval_air(air, local, nxt, public_values, periodic, sels, alpha):
    """air.rs VerifierConstraintFolder over the DAG of a binding.Air with PUBLIC and PERIODIC nodes; periodic: the columns
    at zeta."""
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


def verify(oracle, air, cfg, words, columns=None):
    """-> OK or the code of the first failed check.  words: the flat proof, its air.n_public public values last.
    columns: the periodic columns to check against (default: the AIR's own)."""
    columns = air.periodic_columns if columns is None else columns
    s = Shape(cfg)
    m = int(air.n_public)
    w = [int(x) for x in np.asarray(words, dtype=np.uint64)]
    assert len(w) == s.num_inputs + m and air.width == s.W
    if any(x >= P for x in w):
        return MALFORMED
    public_values = w[s.num_inputs:]

    def permute(state):
        return [int(x) for x in oracle.poseidon2_permute(np.array(state, dtype=np.uint64))[0]]

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
    ch = Challenger(permute)
    ch.observe(trace_root)
    ch.observe(public_values)                                # the extra observe
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
        # every matrix has the height of the LDE domain: one reduced opening per query
        x = GENERATOR * pow(root_of_unity(L), bitrev(index, L), P) % P
        mats = [(row_t, [(zeta, trace_local), (zeta_next, trace_next)])]
        mats += [(rows_q[c], [(zeta, chunks[c])]) for c in range(s.Q)]
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
    folded_constraints = eval_air(air, trace_local, trace_next, public_values, periodic, sels, alpha)
    if e_mul(folded_constraints, inv_zeroifier) != quotient:
        return CONSTRAINTS
    return OK
