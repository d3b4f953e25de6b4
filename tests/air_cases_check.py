"""Traces for the trace checker (include/p25.h "CHECKING A TRACE"): satisfying ones and one-word corruptions of them, by
name.  build(p25, name) -> Case(air, trace, pv, log_n, log_blowup, expect); `expect` holds what the case's construction
says about the report beyond the model's word-for-word statement (tests/p3_check_model.py): verdict, violated
(row, constraint) pairs, counts.

whens      width 2, columns (x, b), two public values:
             c0 when 0: b (b - 1)        c1 when 1: x - PUBLIC(0)
             c2 when 3: x_next - x - b   c3 when 2: x - PUBLIC(1)
           random bits in b, their running sum in x.  Heights 3 (less than a wave), 6, 8 (one block), 9 (two), 12.
           a<r>   b = 2 at row r: c0 and c2 at r            b   x at row 0: c1 and c2 at row 0
           c      x at row n - 1: c3 there, c2 at n - 2 and NOT at n - 1 (the transition is not selected on the last row)
           d      b at row n - 1 flipped: verdict OK, no selected constraint reads it
           e      b = 2 on every row: counts n and n - 1, every lane of every wave voting
aux        tests/air_cases_aux.py: perm (AW 1) and wide (AW 3) at one height below a wave, the scan block exactly and
           twice it, satisfied and with not_a_permutation (the wrap constraint fails on row n - 1 alone); det satisfied and
           with a zero denominator; range, tuple, pvper satisfied.
periodic, preprocessed   one case each of air_cases_periodic.py / air_cases_preprocessed.py, no auxiliary columns: satisfied
           and with one trace word flipped."""
from collections import namedtuple

import numpy as np

import air_cases_aux as aux
import air_cases_periodic as periodic
import air_cases_preprocessed as preprocessed

P = 0xFFFFFFFF00000001
Case = namedtuple("Case", "air trace pv log_n log_blowup expect")
OK, VIOLATED, ZERO_DENOMINATOR = 0, 1, 2


# ---- whens -----------------------------------------------------------------------------------------------------------
def whens(p25):
    air = p25.Air(2, n_public=2)
    x, b, xn = air.local(0), air.local(1), air.next(0)
    air.assert_zero(air.mul(b, air.sub(b, air.const(1))))
    air.when_first_row(air.sub(x, air.public(0)))
    air.when_transition(air.sub(air.sub(xn, x), b))
    air.when_last_row(air.sub(x, air.public(1)))
    return air


def whens_trace(log_n, seed=0):
    n = 1 << log_n
    rng = np.random.default_rng(55000 + 17 * log_n + seed)
    b = rng.integers(0, 2, n, dtype=np.uint64)
    x0 = int(rng.integers(0, P - n, dtype=np.uint64))
    x = (np.uint64(x0) + np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(b[:-1], dtype=np.uint64)])).astype(np.uint64)
    return np.ascontiguousarray(np.stack([x, b], axis=1)), np.array([x0, int(x[-1])], dtype=np.uint64)


WHENS_LOG_N = [3, 6, 8, 9, 12]
A_ROWS = [0, 63, 64, 255, 256]


def _whens_names():
    out = []
    for k in WHENS_LOG_N:
        n = 1 << k
        rows = sorted(set([r for r in A_ROWS if r < n] + [n - 2]))
        out += ["whens%d_ok" % k] + ["whens%d_a%d" % (k, r) for r in rows] + ["whens%d_%s" % (k, v) for v in "bcde"]
    return out


def _whens(p25, name):
    head, variant = name.split("_")
    k = int(head[5:])
    n = 1 << k
    t, pv = whens_trace(k)
    t = t.copy()
    expect = {}
    if variant == "ok":
        expect = {"verdict": OK, "violations": []}
    elif variant[0] == "a":
        r = int(variant[1:])
        t[r, 1] = 2
        expect = {"verdict": VIOLATED, "violations": [(r, 0)] + ([(r, 2)] if r < n - 1 else [])}
    elif variant == "b":
        t[0, 0] = (int(t[0, 0]) + 5) % P
        expect = {"verdict": VIOLATED, "violations": [(0, 1), (0, 2)]}
    elif variant == "c":
        t[n - 1, 0] = (int(t[n - 1, 0]) + 5) % P
        expect = {"verdict": VIOLATED, "violations": [(n - 2, 2), (n - 1, 3)]}
    elif variant == "d":
        t[n - 1, 1] ^= np.uint64(1)
        expect = {"verdict": OK, "violations": []}
    else:
        assert variant == "e"
        t[:, 1] = 2
        expect = {"verdict": VIOLATED, "counts": [n, 0, n - 1, 0], "first": (0, 0)}
    return Case(whens(p25), t, pv, k, 1, expect)


# ---- auxiliary columns -------------------------------------------------------------------------------------------------
_LOG_BLOCK = aux.SCAN_BLOCK.bit_length() - 1
AUX_HEIGHTS = [5, _LOG_BLOCK, _LOG_BLOCK + 1]       # one below a wave, the scan block exactly, twice the scan block


def _aux_names():
    out = []
    for cols in (1, 3):
        for k in AUX_HEIGHTS:
            out += ["perm%d_%d_ok" % (cols, k), "perm%d_%d_notperm" % (cols, k)]
    out += ["det_%d_ok" % AUX_HEIGHTS[0]] + ["det_%d_zero%d" % (k, r) for k in AUX_HEIGHTS for r in (0, (1 << k) - 1)]
    out += ["det_%d_zero%d" % (AUX_HEIGHTS[2], aux.SCAN_BLOCK + 1)]
    out += ["range_%d_ok" % _LOG_BLOCK, "tuple_5_ok", "pvper_%d_ok" % (_LOG_BLOCK + 1)]
    return out


def _aux(p25, name):
    kind, k, variant = name.split("_")
    k = int(k)
    n = 1 << k
    if kind.startswith("perm"):
        cols = int(kind[4:])
        air, t = aux.perm(p25, 0, cols), aux.perm_trace(k)
        if variant == "ok":
            return Case(air, t, None, k, 1, {"verdict": OK, "violations": [], "totals_zero": True})
        # S(n) != 0 = S(0): the running-sum constraint of every column fails where NEXT wraps, and nowhere else
        return Case(air, aux.not_a_permutation(t), None, k, 1,
                    {"verdict": VIOLATED, "violations": [(n - 1, 2 * j + 1) for j in range(cols)], "totals_zero": False})
    if kind == "det":
        air, t = aux.det_air(p25), aux.det_trace(k)
        if variant == "ok":
            return Case(air, t, None, k, 1, {"verdict": OK, "violations": [], "totals_zero": True})
        r = int(variant[4:])
        t = t.copy()
        t[r, 1] = 0
        if r + 3 < n:
            t[r + 3, 1] = 0                          # a later one: the report names the first
        return Case(air, t, None, k, 1, {"verdict": ZERO_DENOMINATOR, "zero": (r, 0)})
    assert variant == "ok"
    ok = {"verdict": OK, "violations": [], "totals_zero": True}
    if kind == "range":
        return Case(aux.range_air(p25, k), aux.range_trace(k), None, k, 1, ok)
    if kind == "tuple":
        return Case(aux.tuple_air(p25), aux.tuple_trace(k), None, k, 1, ok)
    assert kind == "pvper"
    t, pv = aux.pvper_trace(k)
    return Case(aux.pvper_air(p25), t, pv, k, 1, ok)


# ---- periodic / preprocessed columns without auxiliary ones ------------------------------------------------------------
def _tables(p25, name):
    kind, variant = name.split("_")
    if kind == "periodic":
        air, t, pv, k, B = periodic.make(p25, periodic.SHAPES[periodic.SHAPE_IDS.index("mix123")])
    else:
        air, t, pv, _prep, k, B = preprocessed.make(p25, preprocessed.shape("mix4"))
    if variant == "ok":
        return Case(air, t, pv, k, B, {"verdict": OK, "violations": []})
    t = t.copy()
    r = t.shape[0] // 2
    t[r, t.shape[1] - 1] = (int(t[r, t.shape[1] - 1]) + 1) % P
    return Case(air, t, pv, k, B, {"verdict": VIOLATED})


WHENS_NAMES = _whens_names()
AUX_NAMES = _aux_names()
TABLE_NAMES = ["periodic_ok", "periodic_flip", "preprocessed_ok", "preprocessed_flip"]
NAMES = WHENS_NAMES + AUX_NAMES + TABLE_NAMES


def build(p25, name):
    if name in WHENS_NAMES:
        return _whens(p25, name)
    if name in AUX_NAMES:
        return _aux(p25, name)
    return _tables(p25, name)


def check_expectations(case, words):
    """What the case's construction says of a report (the raw words), beyond its equality with the model's."""
    w = [int(x) for x in words]
    aw, nc, ex = len(case.air.aux_columns), len(case.air.constraints), case.expect
    none = (1 << 64) - 1
    counts, totals = w[8 + 2 * aw:], w[8:8 + 2 * aw]
    assert len(counts) == nc and w[6] == w[7] == 0
    assert w[0] == ex["verdict"]
    assert w[1] == sum(counts)
    if "violations" in ex:
        v = sorted(ex["violations"])
        assert counts == [sum(1 for _r, c in v if c == j) for j in range(nc)]
        assert (w[2], w[3]) == (v[0] if v else (none, none))
    if "counts" in ex:
        assert counts == ex["counts"] and (w[2], w[3]) == ex["first"]
    if "zero" in ex:
        assert (w[4], w[5]) == ex["zero"] and w[1:4] == [0, none, none] and not any(totals) and not any(counts)
    else:
        assert (w[4], w[5]) == (none, none)
    if "totals_zero" in ex:
        assert (not any(totals)) == ex["totals_zero"]
