"""AIRs with FREE columns, and traces that put boundary-valued Goldilocks words (tests/edge_values.py) into them.

A boundary-valued trace still has to satisfy its AIR.  AirProgram::validate does not require that a constraint pins a column,
so the AIRs here leave one or two columns free: the fills below go into them as they are, and the other columns are derived
from them in Python integers.  The device prover then runs its LDE, run_air (device gl::mul / add / sub), the quotient, the
openings and FRI on these words and on what the transforms make of them.

base field   free_ops    width 5, a and b free; c = a b, d = a + b, e = a - b on every row.  Degree 2, one chunk.
             free_acc    width 3, a and b free; s = 0 on the first row, next s = s + a b.  Reads NEXT; a transition of degree 3,
                         two chunks.  The last row's a and b are read by no constraint.
             free_pow5   width 2, a free; y = a^5 on every row.  Degree 5, four chunks, log_blowup >= 2.
F_p^2        edge_range  air_cases_aux's `range` LogUp, the preprocessed table the words of EDGE repeated to 2^log_n: f is drawn
                         from it by row, m counts the draws of each row.
             edge_pvper  air_cases_aux's `pvper`, the periodic column and both public values taken from EDGE.

FILLS names the fills of a free column; constant_pairs() lists every ordered pair of EDGE for free_ops' constant traces."""
import numpy as np

import air_cases_aux
import edge_values as ev
from edge_values import EDGE, EPS, P

# ---- fills of a free column: name -> fn(n, seed) ---------------------------------------------------------------------------
FILLS = dict(ev.GENERATORS)
FILLS.update({
    "alternating(p-1,0)": lambda n, _s: ev.alternating(n, P - 1, 0),
    "delta(n-1,p-1)": lambda n, _s: ev.delta(n, n - 1, P - 1),
    "geometric(w_n)": lambda n, _s: ev.geometric(n, ev.root_of_unity(n.bit_length() - 1)),
    "geometric(p-1)": lambda n, _s: ev.geometric(n, P - 1),
    "const(p-1)": lambda n, _s: ev.const(n, P - 1),
    "const(2^32-1)": lambda n, _s: ev.const(n, EPS),
    "const(0)": lambda n, _s: ev.const(n, 0),
})
FILL_NAMES = list(FILLS)


def fill_pairs():
    """(name, fill of a, fill of b): every fill against itself (another seed) and against the fill three places on, so that
    every fill meets its own class and another one in a product."""
    out = []
    for k, name in enumerate(FILL_NAMES):
        other = FILL_NAMES[(k + 3) % len(FILL_NAMES)]
        out += [(f"{name} x {name}", name, name), (f"{name} x {other}", name, other)]
    return out


def _ints(col):
    return [int(v) for v in col]


# ---- free_ops ------------------------------------------------------------------------------------------------------------
def free_ops(p25):
    air = p25.Air(5)
    a, b, c, d, e = (air.local(i) for i in range(5))
    air.assert_zero(air.sub(air.mul(a, b), c))
    air.assert_zero(air.sub(air.add(a, b), d))
    air.assert_zero(air.sub(air.sub(a, b), e))
    return air


def free_ops_trace(a, b):
    a, b = _ints(a), _ints(b)
    return np.array([[x, y, x * y % P, (x + y) % P, (x - y) % P] for x, y in zip(a, b)], dtype=np.uint64)


def constant_pairs():
    """Every ordered pair (u, v) of EDGE."""
    return [(u, v) for u in EDGE for v in EDGE]


def free_ops_constant_traces(log_n):
    """uint64[len(EDGE)^2][2^log_n][5]: the trace of pair k is (u, v, u v, u + v, u - v) on every row."""
    rows = np.array([[u, v, u * v % P, (u + v) % P, (u - v) % P] for u, v in constant_pairs()], dtype=np.uint64)
    return np.ascontiguousarray(np.repeat(rows[:, None, :], 1 << log_n, axis=1))


# ---- free_acc ------------------------------------------------------------------------------------------------------------
def free_acc(p25):
    air = p25.Air(3)
    a, b, s = air.local(0), air.local(1), air.local(2)
    air.when_first_row(s)
    air.when_transition(air.sub(air.next(2), air.add(s, air.mul(a, b))))
    return air


def free_acc_trace(a, b):
    a, b = _ints(a), _ints(b)
    rows, s = [], 0
    for x, y in zip(a, b):
        rows.append([x, y, s])
        s = (s + x * y) % P
    return np.array(rows, dtype=np.uint64)


# ---- free_pow5 -----------------------------------------------------------------------------------------------------------
def free_pow5(p25):
    air = p25.Air(2)
    a, y = air.local(0), air.local(1)
    a2 = air.mul(a, a)
    air.assert_zero(air.sub(air.mul(air.mul(a2, a2), a), y))
    return air


def free_pow5_trace(a, _b=None):
    return np.array([[x, pow(x, 5, P)] for x in _ints(a)], dtype=np.uint64)


# name -> (air maker, trace maker(a, b), constraint degree with the selector, log_blowups)
FAMILIES = {"free_ops": (free_ops, free_ops_trace, 2, (1, 2)),
            "free_acc": (free_acc, free_acc_trace, 3, (1, 2)),
            "free_pow5": (free_pow5, free_pow5_trace, 5, (2, 3))}


def traces(family, log_n, names=None):
    """[(name, trace)] of `family` for every pair of fill_pairs() (or those whose first fill is in `names`)."""
    n = 1 << log_n
    make = FAMILIES[family][1]
    out = []
    for k, (name, fa, fb) in enumerate(fill_pairs()):
        if names is not None and fa not in names:
            continue
        if family == "free_pow5" and fa != fb:       # one free column: the second fill of a pair is not read
            continue
        out.append((name, make(FILLS[fa](n, 700 + 2 * k + log_n), FILLS[fb](n, 701 + 2 * k + log_n))))
    return out


def check_rows(air, trace):
    """The AIR's constraints on every row of the trace, in Python integers (air_cases._eval_nodes' node semantics, written
    out again for the ops these families use): the first (row, constraint) that fails, or None."""
    n = trace.shape[0]
    rows = [_ints(r) for r in trace]
    for r in range(n):
        local, nxt, v = rows[r], rows[(r + 1) % n], []
        for op, a, b, value in air.nodes:
            assert op <= 5, "a base-field AIR without public, periodic or preprocessed reads"
            v.append(local[a] if op == 0 else nxt[a] if op == 1 else value % P if op == 2 else
                     (v[a] + v[b]) % P if op == 3 else (v[a] - v[b]) % P if op == 4 else v[a] * v[b] % P)
        for k, (node, when) in enumerate(air.constraints):
            on = when == 0 or (when == 1 and r == 0) or (when == 2 and r == n - 1) or (when == 3 and r < n - 1)
            if on and v[node] != 0:
                return r, k
    return None


# ---- F_p^2: the LogUp AIRs of air_cases_aux on boundary words --------------------------------------------------------------
def edge_table(log_n):
    """uint64[2^log_n][1]: EDGE, repeated."""
    return np.array([EDGE[i % len(EDGE)] for i in range(1 << log_n)], dtype=np.uint64).reshape(-1, 1)


def edge_range_air(p25, log_n):
    """air_cases_aux.range_air with the table above: num = m (g - f) - (g - t), den = (g - t)(g - f)."""
    air = p25.Air(2, preprocessed=edge_table(log_n), aux=1)
    f, m, t, g = air.local(0), air.local(1), air.prep_local(0), air.challenge(0)
    gf, gt = air.sub(g, f), air.sub(g, t)
    num = air.sub(air.mul(m, gf), gt)
    den = air.mul(gt, gf)
    air.aux_column(num, den)
    air_cases_aux._running_sum_constraints(air, 0, num, den)
    return air


def edge_range_trace(log_n, seed=0):
    """f[i] = table[pick[i]], m[j] = the number of i with pick[i] = j: the table repeats its words, so the draws are counted
    by row, not by value."""
    n = 1 << log_n
    pick = (ev.uniform(n, 800 + log_n + seed) % np.uint64(n)).astype(np.int64)
    m = np.bincount(pick, minlength=n).astype(np.uint64)
    return np.ascontiguousarray(np.stack([edge_table(log_n)[pick, 0], m], axis=1))


EDGE_PERIODIC = np.array([P - 1, 0, EPS, P - EPS, 1 << 63, 1, P - (1 << 32), EPS + 1], dtype=np.uint64)
EDGE_PUBLIC_SHIFT = P - 1           # PUBLIC(0): the challenge is read as g + (p - 1)
assert all(int(v) in EDGE for v in EDGE_PERIODIC) and EDGE_PUBLIC_SHIFT in EDGE


def edge_pvper_air(p25):
    """air_cases_aux.pvper_air with the periodic column EDGE_PERIODIC (period 8)."""
    air = p25.Air(2, n_public=2, periodic=[EDGE_PERIODIC], aux=1)
    f, m, t = air.local(0), air.local(1), air.periodic(0)
    g = air.add(air.challenge(0), air.public(0))
    gf, gt = air.sub(g, f), air.sub(g, t)
    num = air.sub(air.mul(m, gf), gt)
    den = air.mul(gt, gf)
    air.aux_column(num, den)
    air.when_first_row(air.sub(f, air.public(1)))
    air_cases_aux._running_sum_constraints(air, 0, num, den)
    return air


def edge_pvper_trace(log_n, seed=0):
    """-> (trace, public values).  Entry v of the periodic column stands on n / 8 rows: each carries count(v) / (n / 8)."""
    n, period = 1 << log_n, EDGE_PERIODIC.size
    pick = (ev.uniform(n, 900 + log_n + seed) % np.uint64(period)).astype(np.int64)
    f = EDGE_PERIODIC[pick]
    reps_inv = pow(n // period, P - 2, P)
    count = np.bincount(pick, minlength=period)
    m = np.array([int(count[i % period]) * reps_inv % P for i in range(n)], dtype=np.uint64)
    return np.ascontiguousarray(np.stack([f, m], axis=1)), np.array([EDGE_PUBLIC_SHIFT, int(f[0])], dtype=np.uint64)


# the heights of the F_p^2 tests: 2^4 rows, and the first height at which the totals pass of the device's prefix sum takes a
# second tile (air_cases_aux.BIG_SHAPES' rule)
EXT_LOG_SMALL = 4
EXT_LOG_BIG = (air_cases_aux.SCAN_BLOCK * air_cases_aux.TOTALS_TILE).bit_length()


def ext_case(p25, kind, log_n, seed=0):
    """-> (air, trace, public values or None)."""
    if kind == "edge_range":
        return edge_range_air(p25, log_n), edge_range_trace(log_n, seed), None
    assert kind == "edge_pvper"
    trace, pv = edge_pvper_trace(log_n, seed)
    return edge_pvper_air(p25), trace, pv
