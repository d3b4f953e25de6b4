"""AIRs with challenges and auxiliary columns (node ops 10 CHALLENGE / 11 AUX_LOCAL / 12 AUX_NEXT, p25_air_aux;
include/p25.h "AUXILIARY COLUMNS") and traces that satisfy them.

Every auxiliary column j carries the usual pair of constraints: first row AUX_LOCAL(j) = 0, every row
(AUX_NEXT(j) - AUX_LOCAL(j)) den_j - num_j = 0.  NEXT is cyclic, so the pair holds exactly when no denominator vanishes and
the terms num_j / den_j sum to zero over the rows.

perm      width 2, column b a permutation of column a: 1 challenge g, num = a - b, den = (g - a)(g - b), i.e. the term
          1 / (g - a) - 1 / (g - b).  Degree 3 (den times an auxiliary column): two chunks.
          perm(extra = d) multiplies the running-sum constraint by a^d: degree 3 + d, for the shapes at log_blowup 2 and 3.
range     LogUp of trace column f into the preprocessed table t = 0..n-1 with a multiplicity column m:
          num = m (g - f) - (g - t), den = (g - t)(g - f).  Auxiliary columns beside preprocessed ones.
tuple     2 challenges g, h: pairs (x, y) looked up in the table of pairs (tx, ty) held by the trace, multiplicity m, both
          compressed as u + h v; column 0 compresses (x, y), column 1 (y, x): AW = 2.
wide      AW = 3 on the perm trace: column j uses the challenge shifted by the constant j: 6 words a row, beyond the sponge's
          4-word absorb (AW = 1 and 2 are on its other side).
det       no challenge: num = LOCAL(0), den = LOCAL(1).  The running sum is deterministic; a zero in column 1 is a zero
          denominator whatever the transcript says.
pvper     public values and a periodic column beside the auxiliary column: LogUp of f into the periodic column (period 4),
          the challenge shifted by PUBLIC(0), and first row f = PUBLIC(1).

SHAPES lists (id, kind, argument, log_n, log_blowup)."""
import re
from pathlib import Path

import numpy as np

P = 0xFFFFFFFF00000001


def scan_constants():
    """The block size of the device's prefix sum and the tile width of its totals pass, read from p3_kernels.h."""
    src = (Path(__file__).resolve().parent.parent / "plonky2.5_amd" / "csrc" / "p3_kernels.h").read_text()
    out = []
    for name in ("P3_AUX_SCAN_BLOCK", "P3_AUX_TOTALS_TILE"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, name
        out.append(int(m.group(1)))
    return tuple(out)


def _rng(log_n, seed):
    return np.random.default_rng(99000 + 131 * log_n + seed)


def _running_sum_constraints(air, j, num, den, extra=None):
    al, an = air.aux_local(j), air.aux_next(j)
    air.when_first_row(al)
    c = air.sub(air.mul(air.sub(an, al), den), num)
    air.assert_zero(c if extra is None else air.mul(c, extra))


# ---- perm, wide -----------------------------------------------------------------------------------------------------
def perm(p25, extra=0, columns=1):
    air = p25.Air(2, aux=1)
    a, b, g = air.local(0), air.local(1), air.challenge(0)
    mult = None
    for _ in range(extra):
        mult = a if mult is None else air.mul(mult, a)
    for j in range(columns):
        gj = g if j == 0 else air.add(g, air.const(j))
        num = air.sub(a, b)
        den = air.mul(air.sub(gj, a), air.sub(gj, b))
        assert air.aux_column(num, den) == j
        _running_sum_constraints(air, j, num, den, mult)
    return air


def perm_trace(log_n, seed=0):
    n = 1 << log_n
    rng = _rng(log_n, seed)
    a = rng.integers(1, P, n, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([a, a[rng.permutation(n)]], axis=1))


def not_a_permutation(trace):
    """One cell of column b changed: the multisets differ, the terms no longer sum to zero."""
    bad = trace.copy()
    r = trace.shape[0] // 2
    bad[r, 1] = (int(bad[r, 1]) + 1) % P
    return bad


# ---- range ----------------------------------------------------------------------------------------------------------
def range_table(log_n):
    return np.arange(1 << log_n, dtype=np.uint64).reshape(-1, 1)


def range_air(p25, log_n):
    air = p25.Air(2, preprocessed=range_table(log_n), aux=1)
    f, m, t, g = air.local(0), air.local(1), air.prep_local(0), air.challenge(0)
    gf, gt = air.sub(g, f), air.sub(g, t)
    num = air.sub(air.mul(m, gf), gt)
    den = air.mul(gt, gf)
    air.aux_column(num, den)
    _running_sum_constraints(air, 0, num, den)
    return air


def range_trace(log_n, seed=0):
    n = 1 << log_n
    f = _rng(log_n, 10 + seed).integers(0, n, n, dtype=np.uint64)
    m = np.bincount(f.astype(np.int64), minlength=n).astype(np.uint64)
    return np.ascontiguousarray(np.stack([f, m], axis=1))


# ---- tuple ----------------------------------------------------------------------------------------------------------
def tuple_air(p25):
    air = p25.Air(5, aux=2)
    x, y, tx, ty, m = (air.local(c) for c in range(5))
    g, h = air.challenge(0), air.challenge(1)
    for j, (u, v, tu, tv) in enumerate(((x, y, tx, ty), (y, x, ty, tx))):
        c, ct = air.add(u, air.mul(h, v)), air.add(tu, air.mul(h, tv))
        gc, gct = air.sub(g, c), air.sub(g, ct)
        num = air.sub(air.mul(m, gc), gct)
        den = air.mul(gct, gc)
        air.aux_column(num, den)
        _running_sum_constraints(air, j, num, den)
    return air


def tuple_trace(log_n, seed=0):
    n = 1 << log_n
    rng = _rng(log_n, 20 + seed)
    table = rng.integers(0, P, (n, 2), dtype=np.uint64)
    pick = rng.integers(0, n, n)
    m = np.bincount(pick, minlength=n).astype(np.uint64)
    return np.ascontiguousarray(np.concatenate([table[pick], table, m.reshape(-1, 1)], axis=1))


# ---- det ------------------------------------------------------------------------------------------------------------
def det_air(p25):
    air = p25.Air(2)
    num, den = air.local(0), air.local(1)
    air.aux_column(num, den)
    _running_sum_constraints(air, 0, num, den)
    return air


def det_trace(log_n, seed=0):
    """Random a_i, d_i != 0; the last a makes the quotients sum to zero."""
    n = 1 << log_n
    rng = _rng(log_n, 30 + seed)
    a = [int(v) for v in rng.integers(0, P, n, dtype=np.uint64)]
    d = [int(v) for v in rng.integers(1, P, n, dtype=np.uint64)]
    total = sum(x * pow(y, P - 2, P) for x, y in zip(a[:-1], d[:-1])) % P
    a[-1] = (P - total) * d[-1] % P
    return np.ascontiguousarray(np.array([a, d], dtype=np.uint64).T)


# ---- pvper ----------------------------------------------------------------------------------------------------------
PVPER_TABLE = np.array([3, 1 << 40, 77, P - 5], dtype=np.uint64)


def pvper_air(p25):
    air = p25.Air(2, n_public=2, periodic=[PVPER_TABLE], aux=1)
    f, m, t = air.local(0), air.local(1), air.periodic(0)
    g = air.add(air.challenge(0), air.public(0))
    gf, gt = air.sub(g, f), air.sub(g, t)
    num = air.sub(air.mul(m, gf), gt)
    den = air.mul(gt, gf)
    air.aux_column(num, den)
    air.when_first_row(air.sub(f, air.public(1)))
    _running_sum_constraints(air, 0, num, den)
    return air


def pvper_trace(log_n, seed=0):
    """-> (trace, public values).  Table entry v stands on n / 4 rows: each carries count(v) / (n / 4) as its multiplicity."""
    n = 1 << log_n
    pick = _rng(log_n, 40 + seed).integers(0, 4, n)
    f = PVPER_TABLE[pick]
    reps_inv = pow(n // 4, P - 2, P)
    count = np.bincount(pick, minlength=4)
    m = np.array([int(count[i % 4]) * reps_inv % P for i in range(n)], dtype=np.uint64)
    return np.ascontiguousarray(np.stack([f, m], axis=1)), np.array([12345, int(f[0])], dtype=np.uint64)


# ---- the shapes -----------------------------------------------------------------------------------------------------
SCAN_BLOCK, TOTALS_TILE = scan_constants()
_LOG_BLOCK = SCAN_BLOCK.bit_length() - 1
_LOG_TILES = (SCAN_BLOCK * TOTALS_TILE).bit_length() - 1     # the totals pass takes one tile up to here

SHAPES = [
    ("perm", "perm", (0, 1), 3, 1),                       # less than a wave
    ("range", "range", None, 4, 1),
    ("tuple", "tuple", None, 3, 1),
    ("wide", "perm", (0, 3), 3, 1),
    ("det", "det", None, 3, 1),
    ("pvper", "pvper", None, 4, 1),
    ("perm_b2", "perm", (1, 1), 3, 2),                    # degree 4: four chunks
    ("perm_b3", "perm", (3, 1), 3, 3),                    # degree 6: eight chunks
    ("perm_block", "perm", (0, 1), _LOG_BLOCK, 1),        # the scan block exactly
    ("perm_2block", "perm", (0, 1), _LOG_BLOCK + 1, 1),   # ... and twice it
]
SHAPE_IDS = [s[0] for s in SHAPES]
# the last height at which the totals pass takes one tile, and the first at which it takes a second: width-2 perm, proved
# with 2 queries and no proof of work
BIG_SHAPES = [("perm_tile", "perm", (0, 1), _LOG_TILES, 1), ("perm_2tile", "perm", (0, 1), _LOG_TILES + 1, 1)]
BIG_IDS = [s[0] for s in BIG_SHAPES]


def shape(name):
    return (SHAPES + BIG_SHAPES)[(SHAPE_IDS + BIG_IDS).index(name)]


def make(p25, shp, seed=0):
    """-> (air, trace, public values or None, log_n, log_blowup)."""
    _id, kind, arg, log_n, log_blowup = shp
    if kind == "perm":
        return perm(p25, *arg), perm_trace(log_n, seed), None, log_n, log_blowup
    if kind == "range":
        return range_air(p25, log_n), range_trace(log_n, seed), None, log_n, log_blowup
    if kind == "tuple":
        return tuple_air(p25), tuple_trace(log_n, seed), None, log_n, log_blowup
    if kind == "det":
        return det_air(p25), det_trace(log_n, seed), None, log_n, log_blowup
    assert kind == "pvper"
    trace, pv = pvper_trace(log_n, seed)
    return pvper_air(p25), trace, pv, log_n, log_blowup
