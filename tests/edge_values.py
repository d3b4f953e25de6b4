"""Boundary-valued Goldilocks operands for the stage kernels, and plain references in Python integers.

The hot path holds field elements lazily (any u64 congruent to the value) in inline assembly whose rare paths -- a
correction that fires, a carry that crosses the two 32-bit halves, a sum that lands exactly on p -- have probability
about 2^-32 per operation on uniform data.  The generators below put every input word on or next to such a boundary;
the structured fills keep the *intermediate* values of a transform there too (a constant column makes every butterfly
of every NTT pass compute u - u and u + u on equal operands; a delta column keeps all but one operand an exact zero).

No GPU and no oracle here: `splitmix_field` is used as an index source only, and every reference is written with
Python `int` and `pow(.., .., P)` -- no numpy arithmetic on field values.
"""
import os
import re

import numpy as np

from conftest import ROOT, splitmix_field

P = 0xFFFFFFFF00000001
EPS = (1 << 32) - 1                      # 2^64 mod p
TWO_ADIC = 1753635133440165772           # generator of the 2^32-element subgroup
COSET = 7                                # multiplicative generator: the LDE coset shift
INV7 = pow(7, P - 2, P)

# Canonical boundary words: the canonical members of the list in tests/native/lazy_defs.cpp plus the values whose low
# or high 32-bit half is all zeros / all ones.
EDGE = list(dict.fromkeys([                          # (p - EPS - 1 is p - 2^32 again: listed once)
    0, 1, 2, 3, 7, INV7,
    EPS - 1, EPS, EPS + 1, EPS + 2,                  # 0xFFFFFFFE, 0xFFFFFFFF, 2^32, 2^32 + 1
    (1 << 63) - 1, 1 << 63,
    (P - 1) // 2, (P + 1) // 2,
    0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFFFF,
    P - (1 << 32), P - EPS, P - EPS - 1,             # 0xFFFFFFFE00000001, 0xFFFFFFFE00000002
    0xFFFFFFFF00000000,                              # p - 1 again
    P - 3, P - 2, P - 1,
]))
assert all(0 <= v < P for v in EDGE)

# Words a caller might hand in by mistake (section "non-canonical words" of the GPU module): three that are >= p, and
# 2^64 - 2^32 = p - 1, the largest canonical word, as the control that sits right below them
NONCANONICAL = [P, P + 1, (1 << 64) - 1, (1 << 64) - (1 << 32)]


def _arr(words):
    return np.array([int(w) for w in words], dtype=np.uint64)


_EDGE_ARR = _arr(EDGE)
_M32, _M33 = np.uint64(0xFFFFFFFF), np.uint64(0x1FFFFFFFF)


# ---- seeded generators: uint64 arrays, every word < p -------------------------------------------------------------------
# splitmix_field is the index source only: its words pick a member of EDGE or an offset k; none of them is used as a
# field value except in `uniform` and the uniform quarter of `mixed`.  (Index bookkeeping, vectorised: the selections
# below are table look-ups, masks and one subtraction from p - 1 that cannot wrap.)
def uniform(n, seed):
    return splitmix_field(n, seed=seed)


def edge(n, seed):
    """Every word a member of EDGE."""
    return _EDGE_ARR[(splitmix_field(n, seed=seed) % np.uint64(len(EDGE))).astype(np.int64)]


def high(n, seed):
    """p - 1 - k with k < 2^32: the top of the canonical range (high half 0xFFFFFFFE or 0xFFFFFFFF)."""
    return np.uint64(P - 1) - (splitmix_field(n, seed=seed) & _M32)


def low(n, seed):
    """Words below 2^33: the high half is 0 or 1."""
    return splitmix_field(n, seed=seed) & _M33


def mixed(n, seed):
    """A quarter each of edge / high / low / uniform, the class chosen per word by position."""
    out = splitmix_field(n, seed=seed)
    idx = out.copy()
    out[0::4] = _EDGE_ARR[(idx[0::4] % np.uint64(len(EDGE))).astype(np.int64)]
    out[1::4] = np.uint64(P - 1) - (idx[1::4] & _M32)
    out[2::4] = idx[2::4] & _M33
    return out


GENERATORS = {"edge": edge, "high": high, "low": low, "mixed": mixed}


# ---- structured fills ---------------------------------------------------------------------------------------------------
def const(n, v):
    return np.full(n, int(v) % P, dtype=np.uint64)


def delta(n, r, v=1):
    out = np.zeros(n, dtype=np.uint64)
    out[r] = int(v) % P
    return out


def alternating(n, a, b):
    out = np.empty(n, dtype=np.uint64)
    out[0::2] = int(a) % P
    out[1::2] = int(b) % P
    return out


def geometric(n, x):
    """x^i, i < n."""
    out, t = [], 1
    for _ in range(n):
        out.append(t)
        t = t * x % P
    return _arr(out)


# ---- references in Python integers --------------------------------------------------------------------------------------
def root_of_unity(log_n):
    return pow(TWO_ADIC, 1 << (32 - log_n), P)


def columns(n, seed):
    """name -> column of n words: the column classes of the NTT / LDE tests (one per generator, six structured fills)."""
    w = root_of_unity(n.bit_length() - 1)
    cols = {name: gen(n, seed + k) for k, (name, gen) in enumerate(GENERATORS.items())}
    cols.update({"const(p-1)": const(n, P - 1), "const(0)": const(n, 0), "alternating(p-1,0)": alternating(n, P - 1, 0),
                 "delta(n-1,p-1)": delta(n, n - 1, P - 1), "geometric(w)": geometric(n, w),
                 "geometric(p-1)": geometric(n, P - 1)})
    return cols


def bit_reverse(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def bit_reverse_indices(bits):
    """rev[i] for every i < 2^bits, as an index array (indices, not field values)."""
    rev = np.zeros(1 << bits, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(1 << bits, dtype=np.int64) >> b) & 1) << (bits - 1 - b)
    return rev


def intt_naive(values):
    """Coefficients of the polynomial with f(w^i) = values[i]: c_k = n^-1 sum_i values[i] w^(-ik).  O(n^2)."""
    v = [int(x) for x in values]
    n = len(v)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    w_inv = pow(root_of_unity(log_n), P - 2, P)
    n_inv = pow(n, P - 2, P)
    pw = [pow(w_inv, e, P) for e in range(n)]
    return _arr(n_inv * sum(v[i] * pw[i * k % n] for i in range(n)) % P for k in range(n))


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def coset_lde_naive(coeffs, rate_bits):
    """f(7 w_big^i) stored at the bit-reversed index, the layout of p25_lde_commit's lde_out.  O(n * big)."""
    c = [int(x) for x in coeffs]
    bits = (len(c).bit_length() - 1) + rate_bits
    w = root_of_unity(bits)
    out = [0] * (1 << bits)
    x = COSET
    for i in range(1 << bits):
        out[bit_reverse(i, bits)] = horner(c, x)
        x = x * w % P
    return _arr(out)


def ext_mul(x, y):
    """F_p[X] / (X^2 - 7)."""
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def ext_inv(x):
    n = pow((x[0] * x[0] - 7 * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * n % P, (P - x[1]) * n % P)


def horner_ext(coeffs, point, scale=1):
    """sum_k coeffs[k] (scale * point)^k for a base-field polynomial at an extension point: p25_eval_polys."""
    z = (int(point[0]) * int(scale) % P, int(point[1]) * int(scale) % P)
    acc = (0, 0)
    for c in reversed([int(x) for x in coeffs]):
        acc = ext_mul(acc, z)
        acc = ((acc[0] + c) % P, acc[1])
    return acc


# ---- closed forms, affordable at full size ------------------------------------------------------------------------------
def intt_of_const(n, v):
    """iNTT(const(v)) = v * delta(0)."""
    return delta(n, 0, v)


def intt_of_delta(n, r, v):
    """iNTT(delta(r, v))[k] = v n^-1 w^(-rk)."""
    log_n = n.bit_length() - 1
    step = pow(root_of_unity(log_n), (n - r) % n, P)
    return _arr(int(x) * (int(v) * pow(n, P - 2, P) % P) % P for x in geometric(n, step))


def intt_of_geometric(n, j):
    """iNTT(geometric(w^j)) = delta(j): the values of X^j on the subgroup."""
    return delta(n, j % n, 1)


def coset_points(bits):
    """7 w_big^i for i < 2^bits, natural order, as Python ints."""
    w, x, out = root_of_unity(bits), COSET, []
    for _ in range(1 << bits):
        out.append(x)
        x = x * w % P
    return out


def lde_of_monomial(bits, c, k):
    """LDE of the one-coefficient polynomial c X^k on the 2^bits-point coset, at the bit-reversed index:
    c (7 w_big^i)^k = (c 7^k) (w_big^k)^i, a running product."""
    step, x, nat = pow(root_of_unity(bits), k, P), int(c) * pow(COSET, k, P) % P, []
    for _ in range(1 << bits):
        nat.append(x)
        x = x * step % P
    out = np.empty(1 << bits, dtype=np.uint64)
    out[bit_reverse_indices(bits)] = np.array(nat, dtype=np.uint64)
    return out


# ---- thresholds of the transform, read from its source so that the shapes follow them --------------------------------------
def ntt_source_constants():
    """{NTT_FACTOR_LOG, NTT_PRE_TABLE_LOG, TWO_PASS_LOG} of kernels_ntt.hip; TWO_PASS_LOG is the smallest log_n that `split`
    gives two passes (it is written there as the largest single-pass size)."""
    src = open(os.path.join(ROOT, "plonky2.5_amd", "csrc", "kernels_ntt.hip")).read()
    out = {name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
           for name in ("NTT_FACTOR_LOG", "NTT_PRE_TABLE_LOG")}
    one_pass = re.search(r"static void split\(int log_n[^{]*\{\s*if \(log_n <= (\d+)\) \{\s*log_r1 = 0;", src)
    out["TWO_PASS_LOG"] = int(one_pass.group(1)) + 1
    return out


# ---- the high-rate LDE tests (rate_bits 4..8) ----------------------------------------------------------------------------
# The naive LDE costs n * 2^(log_n + rate) Horner steps a column.  log_n 3 takes every rate; log_n 6 the two ends of the
# range, 4 and 8, where all ten columns still run in about 2 s a direction (rates 5..7 as well would double that), so no
# column is cut.
HIGH_RATE_NAIVE = {3: (4, 5, 6, 7, 8), 6: (4, 8)}
# An oracle LDE of 2^18 points and more is dominated by its Merkle tree, and a leaf of more than four words has to be hashed:
# at (12, 8) ten columns take the oracle 15 s, four 5 s, one 4.7 s.  The cases that large keep four columns.
HIGH_RATE_ORACLE_KEEP = ("edge", "mixed", "const(p-1)", "delta(n-1,p-1)")


def high_rate_naive_columns(log_n, seed):
    """(rates, {name: column}) of the Python-integer LDE tests at rates 4..8."""
    return HIGH_RATE_NAIVE[log_n], columns(1 << log_n, seed)


def high_rate_oracle_columns(log_n, rate_bits, seed):
    """{name: column} of the oracle LDE tests at rates 4..8: every column below 2^18 points, four from there."""
    cols = columns(1 << log_n, seed)
    return cols if log_n + rate_bits < 18 else {name: cols[name] for name in HIGH_RATE_ORACLE_KEEP}


def high_rate_closed_forms(log_n, rate_bits):
    """(values_in, coeffs_in) for the full-size LDE tests without an oracle.
    values_in: (name, values, coefficients, LDE or None); coeffs_in: (name, coefficients, LDE).  const(p-1) -> (p-1) delta(0),
    LDE the constant p-1; delta(n-1, p-1) -> -(n^-1) w^k (coefficients only); geometric(w^j) -> delta(j), LDE (7 w_big^i)^j;
    c X^k -> c (7 w_big^i)^k.  Five running products of 2^(log_n + rate_bits) steps in all: X^(n-1) serves twice."""
    n, bits = 1 << log_n, log_n + rate_bits
    w = root_of_unity(log_n)
    x1, xtop = lde_of_monomial(bits, 1, 1), lde_of_monomial(bits, 1, n - 1)
    values_in = [("const(p-1)", const(n, P - 1), intt_of_const(n, P - 1), const(1 << bits, P - 1)),
                 ("delta(n-1,p-1)", delta(n, n - 1, P - 1), intt_of_delta(n, n - 1, P - 1), None),
                 ("geometric(w)", geometric(n, w), intt_of_geometric(n, 1), x1),
                 ("geometric(w^(n-1))", geometric(n, pow(w, n - 1, P)), intt_of_geometric(n, n - 1), xtop)]
    coeffs_in = [("(p-1) X^(n-1)", delta(n, n - 1, P - 1), lde_of_monomial(bits, P - 1, n - 1)),
                 ("(2^32-1) X", delta(n, 1, EPS), lde_of_monomial(bits, EPS, 1)),
                 ("X^(n-1)", delta(n, n - 1, 1), xtop),
                 ("p-1", delta(n, 0, P - 1), const(1 << bits, P - 1)),
                 # 2^63 times a pre-scale factor t has the low word 0 or 2^63 and the high word t >> 1: the borrow of the
                 # reduction (low word below the top half of the high word) fires for every even t
                 ("2^63 X^(n/2+1)", delta(n, n // 2 + 1, 1 << 63), lde_of_monomial(bits, 1 << 63, n // 2 + 1))]
    return values_in, coeffs_in


# ---- the input classes of the partial-product / quotient tests ----------------------------------------------------------
BOUNDARY_CHALLENGES = [0, 1, P - 1, EPS, P - EPS]


def wire_matrices(shape, seed=900):
    """(name, matrix) for the whole-matrix wire classes: one per generator, const(0) and const(p-1)."""
    size = int(shape[0]) * int(shape[1])
    for k, (name, gen) in enumerate(GENERATORS.items()):
        yield name, gen(size, seed + k).reshape(shape)
    yield "const(0)", const(size, 0).reshape(shape)
    yield "const(p-1)", const(size, P - 1).reshape(shape)


def uniform_challenges(seed):
    """(betas, gammas, alphas), two of each, uniform."""
    return splitmix_field(6, seed=seed).reshape(3, 2)


def boundary_challenge_cases(seed=40):
    """(name, betas, gammas, alphas): each of alpha, beta, gamma in turn (both of its two copies) at each boundary value,
    the other two uniform.  beta = gamma = 0 together would make the denominator w + beta * sigma + gamma vanish wherever
    a wire is 0, which is outside the contract (inverting zero): never produced here."""
    for which, row in (("beta", 0), ("gamma", 1), ("alpha", 2)):
        for k, v in enumerate(BOUNDARY_CHALLENGES):
            ch = uniform_challenges(seed + 10 * row + k).copy()
            ch[row, :] = v
            yield f"{which}={v:#x}", ch[0], ch[1], ch[2]


# ---- the input classes of the opening and FRI tests ---------------------------------------------------------------------
OPENING_POINTS = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (P - 1, P - 1), (0, P - 1)]
OPENING_SCALES = [1, P - 1, 0]


def fri_polynomials(log_n):
    """The coefficient classes of the FRI edge tests, coeffs[2][2^log_n] (extension components)."""
    n = 1 << log_n
    top = np.zeros((2, n), dtype=np.uint64)
    top[:, n - 1] = (P - 1, EPS)
    base_only = np.stack([edge(n, 52), const(n, 0)])
    return {"zero": np.zeros((2, n), dtype=np.uint64), "const(p-1)": const(2 * n, P - 1).reshape(2, n),
            "edge": edge(2 * n, 51).reshape(2, n), "top coefficient only": top, "second component zero": base_only}
