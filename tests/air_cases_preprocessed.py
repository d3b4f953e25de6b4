"""AIRs with preprocessed columns (node ops 8 PREP_LOCAL / 9 PREP_NEXT, p25_air_preprocessed; include/p25.h "PREPROCESSED
COLUMNS") and their traces.

prep_machine(d)   the showcase: width 1, two public values, two preprocessed columns -- sel = PREP_LOCAL(0), random bits
                  that are NOT periodic, and c = PREP_LOCAL(1), random words: a little machine whose program is fixed data.
                  First row local0 = PUBLIC(0); last row local0 = PUBLIC(1); transition
                      d = 2   next0 = local0 + sel c                                   degree 3 with its selector: 2 chunks
                      d = 3   next0 = sel (local0 c) + (1 - sel) (local0 + c)          degree 4: 4 chunks
                  with_periodic adds a periodic column of period 4 to the step (next0 = ... + PERIODIC(0)): preprocessed
                  columns, a periodic column and public values in one AIR.
prep_mix(PW)      the sharper one: width 2, PW random columns.  Column 0 counts (next0 = local0 + 1).  On every row
                      local1 = sum_i c_i PREP_LOCAL(i) + local0 PREP_LOCAL(0),
                  and on transitions the same relation differenced, read through PREP_NEXT,
                      next1 - local1 = sum_i c_i (PREP_NEXT(i) - PREP_LOCAL(i)) + next0 PREP_NEXT(0) - local0 PREP_LOCAL(0),
                  with distinct weights c_i (mix_weights), so that a wrong column index, rotation or offset cannot cancel.
                  Degree 3 with the selector: two chunks.

SHAPES lists (id, kind, arguments, log_n, log_blowup): the smallest shapes at which each path of the provers can go wrong."""
import numpy as np

from air_cases_pv import mix_weights

P = 0xFFFFFFFF00000001


def columns(log_n, width, seed=0):
    """Random preprocessed matrix uint64[2^log_n][width]."""
    return np.random.default_rng(88000 + 100 * log_n + 7 * width + seed).integers(0, P, size=(1 << log_n, width), dtype=np.uint64)


# ---- prep_machine ---------------------------------------------------------------------------------------------------
def machine_columns(log_n, seed=0):
    m = columns(log_n, 2, 1000 + seed)
    m[:, 0] &= np.uint64(1)
    if log_n >= 2:          # not periodic, whatever the seed gives: the two halves of the selector differ; and the last
        m[0, 0], m[(1 << log_n) // 2, 0], m[(1 << log_n) - 2, 0] = 0, 1, 1      # transition takes its c whatever d is
    return m


MACHINE_PERIODIC = np.array([5, 0, 11, 0], dtype=np.uint64)


def prep_machine(p25, d, prep, with_periodic=False):
    air = p25.Air(1, n_public=2, periodic=[MACHINE_PERIODIC] if with_periodic else None, preprocessed=prep)
    x, sel, c = air.local(0), air.prep_local(0), air.prep_local(1)
    air.when_first_row(air.sub(x, air.public(0)))
    if d == 2:
        step = air.add(x, air.mul(sel, c))
    else:
        assert d == 3
        not_sel = air.sub(air.const(1), sel)
        step = air.add(air.mul(sel, air.mul(x, c)), air.mul(not_sel, air.add(x, c)))
    if with_periodic:
        step = air.add(step, air.periodic(0))
    air.when_transition(air.sub(air.next(0), step))
    air.when_last_row(air.sub(x, air.public(1)))
    return air


def prep_machine_trace(d, prep, x0, with_periodic=False):
    """-> (trace uint64[n][1], public values [x0, the last row])."""
    n = prep.shape[0]
    t = np.zeros((n, 1), dtype=np.uint64)
    x = int(x0) % P
    for i in range(n):
        t[i, 0] = x
        sel, c = int(prep[i, 0]), int(prep[i, 1])
        x = (x + sel * c) % P if d == 2 else (x * c if sel else x + c) % P
        if with_periodic:
            x = (x + int(MACHINE_PERIODIC[i % 4])) % P
    return t, np.array([int(t[0, 0]), int(t[n - 1, 0])], dtype=np.uint64)


# ---- prep_mix -------------------------------------------------------------------------------------------------------
def prep_mix(p25, prep):
    pw = prep.shape[1]
    air = p25.Air(2, preprocessed=prep)
    x, y = air.local(0), air.local(1)
    air.when_transition(air.sub(air.next(0), air.add(x, air.const(1))))
    w = mix_weights(pw)
    acc = None
    for i, c in enumerate(w):
        term = air.mul(air.const(c), air.prep_local(i))
        acc = term if acc is None else air.add(acc, term)
    air.assert_zero(air.sub(y, air.add(acc, air.mul(x, air.prep_local(0)))))
    diff = None
    for i, c in enumerate(w):
        term = air.mul(air.const(c), air.sub(air.prep_next(i), air.prep_local(i)))
        diff = term if diff is None else air.add(diff, term)
    diff = air.add(diff, air.sub(air.mul(air.next(0), air.prep_next(0)), air.mul(x, air.prep_local(0))))
    air.when_transition(air.sub(air.sub(air.next(1), y), diff))
    return air


def prep_mix_trace(prep, start=5):
    n, pw = prep.shape
    w = mix_weights(pw)
    t = np.zeros((n, 2), dtype=np.uint64)
    for r in range(n):
        x = (int(start) + r) % P
        row = [int(v) for v in prep[r]]
        t[r, 0] = x
        t[r, 1] = (sum(c * v for c, v in zip(w, row)) + x * row[0]) % P
    return t


# ---- the shapes -----------------------------------------------------------------------------------------------------
# (id, kind, arguments, log_n, log_blowup).  The MMCS sponge absorbs 4 words per permutation (hash_iter_slices, RATE = 4) and a
# leaf of up to 8 words is two permutations: PW = 1, 4 | 5 and 8 | 9 stand on either side of each boundary.
SHAPES = [
    ("mix1", "mix", 1, 3, 1),                    # one column; log_n 3 at log_blowup 1
    ("mix4", "mix", 4, 3, 1),                    # a leaf of exactly one absorb
    ("mix5", "mix", 5, 2, 1),                    # ... and one word more
    ("mix8", "mix", 8, 3, 2),                    # two absorbs exactly; log_blowup 2
    ("mix9", "mix", 9, 3, 3),                    # three; log_blowup 3
    ("mix2_b4", "mix", 2, 3, 4),                 # log_blowup 4: the LDE made as two interleaved sets of 8 cosets
    ("machine2", "machine", (2, False), 3, 1),   # Q = 2, public values
    ("machine3", "machine", (3, False), 3, 2),   # Q = 4
    ("machine2_n8", "machine", (2, False), 8, 1),   # n Q = 512: two blocks of the quotient kernel
    ("machine2_per", "machine", (2, True), 4, 1),   # with a periodic column and public values
    ("mix64", "mix", 64, 4, 1),                  # the cap
]
SHAPE_IDS = [s[0] for s in SHAPES]


def shape(name):
    return SHAPES[SHAPE_IDS.index(name)]


def make(p25, shp, x0=3, prep=None):
    """-> (air, trace, public values or None, preprocessed matrix, log_n, log_blowup); prep: other columns than the shape's
    own (the trace is computed under them)."""
    _id, kind, args, log_n, log_blowup = shp
    if kind == "machine":
        d, with_periodic = args
        prep = machine_columns(log_n) if prep is None else prep
        trace, pv = prep_machine_trace(d, prep, x0, with_periodic)
        return prep_machine(p25, d, prep, with_periodic), trace, pv, prep, log_n, log_blowup
    prep = columns(log_n, args) if prep is None else prep
    return prep_mix(p25, prep), prep_mix_trace(prep, start=x0 + 2), None, prep, log_n, log_blowup
