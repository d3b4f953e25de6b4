"""AIRs with periodic columns (node op 7 PERIODIC, p25_air_periodic; include/p25.h "PERIODIC COLUMNS") and their traces.

mimc(k, d)        a MiMC-like chain, the showcase: width 1, two public values, one column of period 2^k holding round
                  constants.  First row local0 = PUBLIC(0); transition next0 = (local0 + PERIODIC(0))^d; last row
                  local0 = PUBLIC(1).  The transition constraint has degree d + 1 with its selector, so d = 2 gives
                  log_quotient_degree 1 (two chunks), d = 3 gives 2 (four), d = 5 gives 3 (eight).
per_mix(periods)  width 2, one column per entry of `periods` (its log period).  Column 0 counts (next0 = local0 + 1); on
                  every row local1 = sum_i c_i PERIODIC(i) + local0 PERIODIC(0) with distinct weights c_i, so that a wrong
                  index, table or offset cannot cancel.  The first column of period 4 is the selector (1, 0, 0, 0); every
                  other value is random, fixed by seed.

SHAPES lists (name, AIR arguments, log_n, log_blowup): the smallest shapes at which each path of the provers can go wrong."""
import numpy as np

from air_cases_pv import mix_weights

P = 0xFFFFFFFF00000001


def _column(k, seed):
    return np.random.default_rng(77000 + seed).integers(0, P, size=1 << k, dtype=np.uint64)


# ---- mimc -----------------------------------------------------------------------------------------------------------
def mimc_constants(k, seed=0):
    return _column(k, 100 * k + seed)


def mimc(p25, k, d, constants=None):
    rc = mimc_constants(k) if constants is None else np.asarray(constants, dtype=np.uint64)
    air = p25.Air(1, n_public=2, periodic=[rc])
    x = air.local(0)
    air.when_first_row(air.sub(x, air.public(0)))
    s = air.add(x, air.periodic(0))
    y = s
    for _ in range(d - 1):
        y = air.mul(y, s)
    air.when_transition(air.sub(air.next(0), y))
    air.when_last_row(air.sub(x, air.public(1)))
    return air


def mimc_trace(log_n, k, d, x0, constants=None):
    """-> (trace uint64[2^log_n][1], public values [x0, the last row])."""
    rc = [int(v) for v in (mimc_constants(k) if constants is None else constants)]
    n = 1 << log_n
    t = np.zeros((n, 1), dtype=np.uint64)
    x = int(x0) % P
    for i in range(n):
        t[i, 0] = x
        x = pow((x + rc[i % len(rc)]) % P, d, P)
    return t, np.array([int(t[0, 0]), int(t[n - 1, 0])], dtype=np.uint64)


# ---- per_mix --------------------------------------------------------------------------------------------------------
def per_mix_columns(periods):
    cols, have_selector = [], False
    for i, k in enumerate(periods):
        if k == 2 and not have_selector:
            cols.append(np.array([1, 0, 0, 0], dtype=np.uint64))
            have_selector = True
        else:
            cols.append(_column(k, 1000 * len(periods) + i))
    return cols


def per_mix(p25, periods, columns=None):
    cols = per_mix_columns(periods) if columns is None else columns
    air = p25.Air(2, periodic=cols)
    x, y = air.local(0), air.local(1)
    air.when_transition(air.sub(air.next(0), air.add(x, air.const(1))))
    acc = None
    for i, c in enumerate(mix_weights(len(cols))):
        term = air.mul(air.const(c), air.periodic(i))
        acc = term if acc is None else air.add(acc, term)
    air.assert_zero(air.sub(y, air.add(acc, air.mul(x, air.periodic(0)))))
    return air


def per_mix_trace(log_n, periods, start=5, columns=None):
    cols = [[int(v) for v in c] for c in (per_mix_columns(periods) if columns is None else columns)]
    w = mix_weights(len(cols))
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    for r in range(1 << log_n):
        x = (int(start) + r) % P
        t[r, 0] = x
        t[r, 1] = (sum(c * col[r % len(col)] for c, col in zip(w, cols)) + x * cols[0][r % len(cols[0])]) % P
    return t


# ---- the shapes -----------------------------------------------------------------------------------------------------
# (id, kind, arguments, log_n, log_blowup).  A mimc(k, d) case runs at the smallest log_blowup its degree d + 1 admits.
SHAPES = [
    ("mix1", "per_mix", [1], 1, 1),              # one row pair, P = n = 2: the table wraps exactly once, n/P = 1 (no squaring)
    ("mix123", "per_mix", [1, 2, 3], 3, 1),      # P = n and P < n side by side; n/P = 4, 2, 1
    ("mimc2_2", "mimc", (2, 2), 3, 1),           # Q = 2: table of P Q = 8 on the quotient coset
    ("mimc2_3", "mimc", (2, 3), 3, 2),           # Q = 4: table of 16
    ("mimc3_5", "mimc", (3, 5), 4, 3),           # Q = 8
    ("mimc8_2", "mimc", (8, 2), 8, 1),           # n Q = 512: two blocks of the quotient kernel; the greatest period
    ("mimc8_3", "mimc", (8, 3), 8, 2),           # n Q = 1024: four blocks
    ("mix8x32", "per_mix", [8] * 32, 8, 1),      # 32 columns x 256 values: the caps
]
SHAPE_IDS = [s[0] for s in SHAPES]


def make(p25, shape, x0=3):
    """-> (air, trace, public values or None, log_n, log_blowup)"""
    _id, kind, args, log_n, log_blowup = shape
    if kind == "mimc":
        k, d = args
        trace, pv = mimc_trace(log_n, k, d, x0)
        return mimc(p25, k, d), trace, pv, log_n, log_blowup
    return per_mix(p25, args), per_mix_trace(log_n, args), None, log_n, log_blowup
