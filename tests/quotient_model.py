"""Z / partial products and the quotient polynomials of a circuit in Python integers, from a `MiniCircuit.build()` dictionary
and tests/gate_models.py -- what p25_partial_products and p25_quotient compute, restated from upstream's definitions
(prover.rs `wires_permutation_partial_products_and_zs`, `compute_quotient_polys`; vanishing_poly.rs).  Neither the oracle nor
the library is called.

Matrices are lists of columns (or numpy arrays [columns][n]); results are lists of lists of Python integers.
"""
import gate_models as gm
from blob_writer import P, UNUSED_SELECTOR, root_of_unity

COSET = 7
QDF = 8                                                # max_quotient_degree_factor = 2^min(rate_bits, 3), rate_bits >= 3


# ---- radix-2 NTT, natural order in and out ----------------------------------------------------------------------------------
def _fft(a, roots):
    """a(roots[1]^i) for i < len(a); roots = the powers of a primitive len(a)-th root, the first half of them."""
    n = len(a)
    if n == 1:
        return a
    h = n // 2
    ev, od = _fft(a[0::2], roots[0::2]), _fft(a[1::2], roots[0::2])
    t = [roots[i] * od[i] % P for i in range(h)]
    return [(ev[i] + t[i]) % P for i in range(h)] + [(ev[i] - t[i]) % P for i in range(h)]


_roots = {}


def _half_roots(log_n, inverse=False):
    key = (log_n, inverse)
    if key not in _roots:
        w = root_of_unity(log_n)
        if inverse:
            w = pow(w, P - 2, P)
        out, x = [], 1
        for _ in range(max(1, (1 << log_n) // 2)):
            out.append(x)
            x = x * w % P
        _roots[key] = out
    return _roots[key]


def ntt(coeffs):
    return _fft(list(coeffs), _half_roots(len(coeffs).bit_length() - 1))


def intt(values):
    n = len(values)
    inv_n = pow(n, P - 2, P)
    return [v * inv_n % P for v in _fft(list(values), _half_roots(n.bit_length() - 1, True))]


def coset_lde(values, factor):
    """Values on <w_n> -> values on COSET <w_(factor n)>, natural order."""
    n = len(values)
    c = intt([int(v) for v in values])
    shifted, s = [], 1
    for v in c:
        shifted.append(v * s % P)
        s = s * COSET % P
    return ntt(shifted + [0] * (n * (factor - 1)))


def coset_interpolate(values):
    """Values on COSET <w_m> -> the m coefficients."""
    c = intt(values)
    inv, s, out = pow(COSET, P - 2, P), 1, []
    for v in c:
        out.append(v * s % P)
        s = s * inv % P
    return out


# ---- the permutation argument --------------------------------------------------------------------------------------------
def _chunks(num_routed):
    return [range(j, min(j + QDF, num_routed)) for j in range(0, num_routed, QDF)]


def partial_products(b, wires, betas, gammas):
    """Rows Z_0, Z_1, then the partial products of challenge 0 (NP rows), then those of challenge 1; NP = chunks - 1, a chunk
    QDF routed wires (the last one what is left).  Z(1) = 1, Z(w x) = Z(x) prod_j (w_j + beta k_j x + gamma) / (w_j + beta
    sigma_j(x) + gamma); partial product k at x is Z(x) times the quotients of the chunks 0..k.  Raises ZeroDivisionError on
    a zero denominator."""
    n = 1 << b["degree_bits"]
    chunks = _chunks(b["num_routed"])
    w_n = root_of_unity(b["degree_bits"])
    zs, pps = [], []
    for beta, gamma in zip((int(v) for v in betas), (int(v) for v in gammas)):
        z_col, pp_cols, z, x = [], [[] for _ in chunks[:-1]], 1, 1
        for r in range(n):
            z_col.append(z)
            for k, chunk in enumerate(chunks):
                for j in chunk:
                    wv = int(wires[j][r])
                    den = (wv + beta * b["sigmas"][j][r] + gamma) % P
                    if den == 0:
                        raise ZeroDivisionError(f"row {r} routed wire {j}")
                    z = z * ((wv + beta * b["k_is"][j] * x + gamma) % P) % P * pow(den, P - 2, P) % P
                if k < len(chunks) - 1:
                    pp_cols[k].append(z)
            x = x * w_n % P
        zs.append(z_col)
        pps += pp_cols
    return zs + pps


# ---- the quotient ----------------------------------------------------------------------------------------------------------
def _circuit_ldes(b):
    if "_ldes" not in b:
        b["_ldes"] = {name: [coset_lde(col, QDF) for col in b[name]] for name in ("selectors", "const_polys", "sigmas")}
    return b["_ldes"]


def filters(b, F, selector_values):
    """filter_g = prod_(k in g's group, k != g) (k - s) [times (UNUSED - s) with more than one selector polynomial], s the value
    of g's selector polynomial: one per gate of b["kinds"]."""
    out = []
    for g in range(len(b["kinds"])):
        s = selector_values[b["group_of"][g]]
        lo, hi = b["groups"][b["group_of"][g]]
        f = F.one
        for k in range(lo, hi):
            if k != g:
                f = F.mul(f, F.sub(F.k(k), s))
        if len(b["selectors"]) > 1:
            f = F.mul(f, F.sub(F.k(UNUSED_SELECTOR), s))
        out.append(f)
    return out


def vanishing_terms(b, F, x, l0, consts, sigmas, wires, zs, zs_next, pps, betas, gammas, pi_hash):
    """The terms of the vanishing polynomial at one point, in the order both alphas fold them: L_0(x) (Z_c(x) - 1) for c = 0, 1;
    the chunk checks of challenge 0, then of challenge 1 (prev num - next den, from Z(x) through the partial products to
    Z(w x)); then for every constraint index j the sum over the gates of filter_g c_(g, j).  consts = selector values, then
    the two gate constants; pps[c] the partial products of challenge c; everything an element of F."""
    ns = len(b["selectors"])
    chunks = _chunks(b["num_routed"])
    terms = [F.mul(l0, F.sub(zs[c], F.one)) for c in range(2)]
    for c in range(2):
        beta, gamma = F.k(int(betas[c])), F.k(int(gammas[c]))
        chain = [zs[c]] + list(pps[c]) + [zs_next[c]]
        for k, chunk in enumerate(chunks):
            num = den = F.one
            for j in chunk:
                wg = F.add(wires[j], gamma)
                num = F.mul(num, F.add(wg, F.mul(beta, F.scale(x, b["k_is"][j]))))
                den = F.mul(den, F.add(wg, F.mul(beta, sigmas[j])))
            terms.append(F.sub(F.mul(chain[k], num), F.mul(chain[k + 1], den)))
    gate_terms = [F.zero] * max([0] + [gm.bw.GATE_CONSTRAINTS[k] for k in b["kinds"]])
    for kind, f in zip(b["kinds"], filters(b, F, consts[:ns])):
        for j, c in enumerate(gm.constraints(kind, F, wires, consts[ns], consts[ns + 1], pi_hash)):
            gate_terms[j] = F.add(gate_terms[j], F.mul(f, c))
    return terms + gate_terms


def fold(F, terms, alpha):
    """sum_j alpha^j terms[j]."""
    acc, a = F.zero, F.k(int(alpha))
    for t in reversed(terms):
        acc = F.add(F.mul(acc, a), t)
    return acc


def quotient(b, wires, zs_pp, betas, gammas, alphas):
    """The vanishing polynomial of each alpha on the 8n points COSET w_(8n)^i, divided by x^n - 1, interpolated there and cut
    into 8 chunks of n coefficients: rows chunk 0..7 of alpha 0, then of alpha 1.  zs_pp as partial_products returns it; the
    PublicInputGate compares with columns 0..3 of row b["pi_row"] of `wires`."""
    F = gm.Base
    n = 1 << b["degree_bits"]
    big = QDF * n
    np_ = len(_chunks(b["num_routed"])) - 1
    assert len(zs_pp) == 2 * (1 + np_) and len(wires) == b["num_wires"]
    ld = _circuit_ldes(b)
    used = max(b["num_routed"], gm.num_wires_read(b["kinds"]))
    assert used <= b["num_wires"]
    w_lde = [coset_lde(wires[j], QDF) for j in range(used)]
    z_lde = [coset_lde(col, QDF) for col in zs_pp]
    pi_hash = [int(wires[i][b["pi_row"]]) for i in range(4)]
    w_big = root_of_unity(b["degree_bits"] + 3)
    inv_n = pow(n, P - 2, P)
    values = [[], []]
    x = COSET
    for i in range(big):
        nxt = (i + QDF) % big                                   # the point w_n x
        zh = (pow(x, n, P) - 1) % P
        l0 = zh * inv_n % P * pow((x - 1) % P, P - 2, P) % P   # L_0(x) = (x^n - 1) / (n (x - 1))
        terms = vanishing_terms(
            b, F, x, l0, [col[i] for col in ld["selectors"] + ld["const_polys"]], [col[i] for col in ld["sigmas"]],
            [col[i] for col in w_lde], [z_lde[c][i] for c in range(2)], [z_lde[c][nxt] for c in range(2)],
            [[z_lde[2 + c * np_ + k][i] for k in range(np_)] for c in range(2)], betas, gammas, pi_hash)
        zh_inv = pow(zh, P - 2, P)
        for c in range(2):
            values[c].append(fold(F, terms, alphas[c]) * zh_inv % P)
        x = x * w_big % P
    out = []
    for c in range(2):
        coeffs = coset_interpolate(values[c])
        out += [coeffs[k * n:(k + 1) * n] for k in range(QDF)]
    return out
