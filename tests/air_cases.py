"""User AIRs for the 8f-2 tests (data form of the reference's `Air` trait, src/p3/air.rs:10-18) with
trace generators.  Constraint degree (selector included) <= 2: one quotient chunk, what the reference's proof model holds
(serde/proof.rs:41-48); the `cubic*` AIRs at the end have degree 3: two chunks (round 5)."""
import numpy as np

P = 0xFFFFFFFF00000001


def fib_trace(log_n):
    n = 1 << log_n
    t = np.zeros((n, 3), dtype=np.uint64)
    a, b = 1, 1
    for i in range(n):
        c = (a + b) % P
        t[i] = (a, b, c)
        a, b = b, c
    return t


def tribonacci(p25):
    """width 4: d = a + b + c on every row; (a, b, c) <- (b, c, d); first row (1, 1, 2); last row pins nothing."""
    air = p25.Air(4)
    a, b, c, d = (air.local(i) for i in range(4))
    na, nb, nc = air.next(0), air.next(1), air.next(2)
    air.assert_zero(air.sub(air.add(air.add(a, b), c), d))
    one, two = air.const(1), air.const(2)
    air.when_first_row(air.sub(a, one))
    air.when_first_row(air.sub(b, one))
    air.when_first_row(air.sub(c, two))
    air.when_transition(air.sub(na, b))
    air.when_transition(air.sub(nb, c))
    air.when_transition(air.sub(nc, d))
    return air


def tribonacci_trace(log_n):
    n = 1 << log_n
    t = np.zeros((n, 4), dtype=np.uint64)
    a, b, c = 1, 1, 2
    for i in range(n):
        d = (a + b + c) % P
        t[i] = (a, b, c, d)
        a, b, c = b, c, d
    return t


def squares(p25):
    """width 3 with a quadratic always-constraint and a last-row constraint:
    s = x * x on every row; x <- x + 3; first row x = 5; last row: y = x (y free elsewhere)."""
    air = p25.Air(3)
    x, s, y = air.local(0), air.local(1), air.local(2)
    nx = air.next(0)
    air.assert_zero(air.sub(air.mul(x, x), s))
    air.when_first_row(air.sub(x, air.const(5)))
    air.when_transition(air.sub(nx, air.add(x, air.const(3))))
    air.when_last_row(air.sub(y, x))
    return air


def squares_trace(log_n, seed=1):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 3), dtype=np.uint64)
    x = 5
    for i in range(n):
        t[i] = (x, (x * x) % P, int(rng.integers(0, P, dtype=np.uint64)))
        x = (x + 3) % P
    t[n - 1, 2] = t[n - 1, 0]
    return t


def random_recurrence(p25, seed, width):
    """A seeded FAMILY of AIRs of any width (docs/DEVELOPER-GUIDE.md's recipe, generated): column j of the next row is
    b_j * local[r_j] + c_j with random r_j, b_j, c_j (a transition constraint per column), the first row is pinned to
    random constants.  Returns (air, coefficients); random_recurrence_trace builds the trace from the coefficients."""
    rng = np.random.default_rng(seed)
    air = p25.Air(width)
    coef = []
    for j in range(width):
        rj = int(rng.integers(0, width))
        bj, cj, first = (int(v) for v in rng.integers(1, P, size=3, dtype=np.uint64))
        coef.append((rj, bj, cj, first))
        air.when_first_row(air.sub(air.local(j), air.const(first)))
        air.when_transition(air.sub(air.next(j), air.add(air.mul(air.const(bj), air.local(rj)), air.const(cj))))
    return air, coef


def random_recurrence_trace(coef, log_n):
    n, width = 1 << log_n, len(coef)
    t = np.zeros((n, width), dtype=np.uint64)
    row = [c[3] for c in coef]
    for i in range(n):
        t[i] = row
        row = [(c[1] * row[c[0]] + c[2]) % P for c in coef]
    return t


def quadratic_pair(p25, seed):
    """width 4, seeded: (x, y) evolve linearly with random coefficients, s = x * y and u = (x + y) * (x + k) hold on EVERY
    row (degree-2 always-constraints).  Exercises two independent quadratic constraints with random constants through
    the verifier circuit's constraint folding."""
    rng = np.random.default_rng(seed)
    a, b, c, d, e, f, k, x0, y0 = (int(v) for v in rng.integers(1, P, size=9, dtype=np.uint64))
    air = p25.Air(4)
    x, y, s, u = (air.local(i) for i in range(4))
    air.assert_zero(air.sub(air.mul(x, y), s))
    air.assert_zero(air.sub(air.mul(air.add(x, y), air.add(x, air.const(k))), u))
    air.when_first_row(air.sub(x, air.const(x0)))
    air.when_first_row(air.sub(y, air.const(y0)))
    air.when_transition(air.sub(air.next(0), air.add(air.add(air.mul(air.const(a), x), air.mul(air.const(b), y)), air.const(c))))
    air.when_transition(air.sub(air.next(1), air.add(air.add(air.mul(air.const(d), x), air.mul(air.const(e), y)), air.const(f))))
    return air, (a, b, c, d, e, f, k, x0, y0)


def quadratic_pair_trace(par, log_n):
    a, b, c, d, e, f, k, x, y = par
    n = 1 << log_n
    t = np.zeros((n, 4), dtype=np.uint64)
    for i in range(n):
        t[i] = (x, y, x * y % P, (x + y) * (x + k) % P)
        x, y = (a * x + b * y + c) % P, (d * x + e * y + f) % P
    return t


def cubic(p25):
    """width 2, degree 3 in an ALWAYS constraint: y = x^3 on every row; x <- y + 1; first row x = 2.  Two quotient chunks."""
    air = p25.Air(2)
    x, y = air.local(0), air.local(1)
    air.assert_zero(air.sub(air.mul(air.mul(x, x), x), y))
    air.when_first_row(air.sub(x, air.const(2)))
    air.when_transition(air.sub(air.next(0), air.add(y, air.const(1))))
    return air


def cubic_trace(log_n):
    n = 1 << log_n
    t = np.zeros((n, 2), dtype=np.uint64)
    x = 2
    for i in range(n):
        y = pow(x, 3, P)
        t[i] = (x, y)
        x = (y + 1) % P
    return t


def cubic_transition(p25):
    """width 3, degree 3 through the SELECTOR: the transition constraint next x = x * y + 5 is quadratic, times
    is_transition; y <- y + x (linear), z = x * y on every row (degree 2), last row: z pinned to x * y through a second
    route (z - x y is already zero: the constraint z - x*y under when_last_row has degree 3 as well)."""
    air = p25.Air(3)
    x, y, z = air.local(0), air.local(1), air.local(2)
    air.assert_zero(air.sub(air.mul(x, y), z))
    air.when_first_row(air.sub(x, air.const(3)))
    air.when_first_row(air.sub(y, air.const(7)))
    air.when_transition(air.sub(air.next(0), air.add(air.mul(x, y), air.const(5))))
    air.when_transition(air.sub(air.next(1), air.add(y, x)))
    air.when_last_row(air.sub(air.mul(x, y), z))
    return air


def cubic_transition_trace(log_n):
    n = 1 << log_n
    t = np.zeros((n, 3), dtype=np.uint64)
    x, y = 3, 7
    for i in range(n):
        t[i] = (x, y, x * y % P)
        x, y = (x * y + 5) % P, (y + x) % P
    return t


def quartic_map(p25, seed):
    """Seeded family, constraint degree 4 in an ALWAYS constraint (FOUR quotient chunks, needs log_blowup >= 2):
    width 2, y = x^4 + a x + b on every row; next x = y + c x (transition); first row x = x0.  Returns (air, (a, b, c, x0))."""
    rng = np.random.default_rng(seed)
    a, b, c, x0 = (int(v) for v in rng.integers(1, P, size=4, dtype=np.uint64))
    air = p25.Air(2)
    x, y = air.local(0), air.local(1)
    x2 = air.mul(x, x)
    x4 = air.mul(x2, x2)
    air.assert_zero(air.sub(air.add(air.add(x4, air.mul(air.const(a), x)), air.const(b)), y))
    air.when_first_row(air.sub(x, air.const(x0)))
    air.when_transition(air.sub(air.next(0), air.add(y, air.mul(air.const(c), x))))
    return air, (a, b, c, x0)


def quartic_map_trace(par, log_n):
    a, b, c, x = par
    n = 1 << log_n
    t = np.zeros((n, 2), dtype=np.uint64)
    for i in range(n):
        y = (pow(x, 4, P) + a * x + b) % P
        t[i] = (x, y)
        x = (y + c * x) % P
    return t


def quintic_selector(p25, seed):
    """Seeded family, constraint degree 5 THROUGH THE SELECTOR (four quotient chunks): width 3, the transition constraint
    next x = x^2 y^2 + k is quartic, times is_transition; next y = y + d x; z = x y on every row (degree 2); the last row pins
    z - x y once more under when_last_row (degree 3).  Returns (air, (k, d, x0, y0))."""
    rng = np.random.default_rng(seed)
    k, d, x0, y0 = (int(v) for v in rng.integers(1, P, size=4, dtype=np.uint64))
    air = p25.Air(3)
    x, y, z = air.local(0), air.local(1), air.local(2)
    air.assert_zero(air.sub(air.mul(x, y), z))
    air.when_first_row(air.sub(x, air.const(x0)))
    air.when_first_row(air.sub(y, air.const(y0)))
    xy = air.mul(x, y)
    air.when_transition(air.sub(air.next(0), air.add(air.mul(xy, xy), air.const(k))))
    air.when_transition(air.sub(air.next(1), air.add(y, air.mul(air.const(d), x))))
    air.when_last_row(air.sub(air.mul(x, y), z))
    return air, (k, d, x0, y0)


def quintic_selector_trace(par, log_n):
    k, d, x, y = par
    n = 1 << log_n
    t = np.zeros((n, 3), dtype=np.uint64)
    for i in range(n):
        t[i] = (x, y, x * y % P)
        x, y = (pow(x * y % P, 2, P) + k) % P, (y + d * x) % P
    return t


# ---------------------------------------------------------------------------------------------------------------------
# Generated AIRs for the register program of the device prover (P3AirDevice::compile, run_air)
# ---------------------------------------------------------------------------------------------------------------------
DAG_CONSTS = (0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32)


def _eval_nodes(nodes, count, local, nxt):
    """Values of the first `count` nodes of an Air (op, a, b, value) on one row pair, in Python integers."""
    v = [0] * count
    for i in range(count):
        op, a, b, value = nodes[i]
        if op == 0:
            v[i] = local[a]
        elif op == 1:
            v[i] = nxt[a]
        elif op == 2:
            v[i] = value
        elif op == 3:
            v[i] = (v[a] + v[b]) % P
        elif op == 4:
            v[i] = (v[a] - v[b]) % P
        else:
            v[i] = v[a] * v[b] % P
    return v


def random_dag(p25, seed, n_inputs, n_defined, n_ops, max_degree, log_n):
    """A seeded expression DAG with SHARING -> (air, trace).  Columns 0 .. n_inputs-1 are free; the operand pool is
    local(i) of every input column, next(i) of every other one and constants (0, 1, 2, p-1, p-2, 2^32-1, 2^32, three random
    words).  n_ops nodes are a random add / sub / mul of two earlier entries: half the draws take one of the last eight
    arithmetic nodes, a quarter any arithmetic node however old, a quarter a leaf, so many values stay alive at once, are
    read long after they were made, and x op x occurs; a node whose degree would pass max_degree is drawn again.
    n_defined roots are drawn WITH replacement among the arithmetic nodes (a root may be shared by constraints and be an
    interior operand of a later node); defined column j carries root_j - local(n_inputs + j) under a random `when`
    (always where the selector's degree does not fit), the constraints in shuffled order.  The trace holds the root's
    value (next of the last row = the first row) where the constraint is enforced and a random word elsewhere."""
    rng = np.random.default_rng(seed)
    n, width = 1 << log_n, n_inputs + n_defined
    air = p25.Air(width)
    deg = {}
    leaves = []
    for i in range(n_inputs):
        leaves.append(air.local(i))
        deg[leaves[-1]] = 1
        if i % 2 == 0:
            leaves.append(air.next(i))
            deg[leaves[-1]] = 1
    for c in DAG_CONSTS + tuple(int(v) for v in rng.integers(0, P, size=3, dtype=np.uint64)):
        leaves.append(air.const(c))
        deg[leaves[-1]] = 0
    arith = []

    def pick():
        u = rng.random()
        if arith and u < 0.5:
            return arith[-1 - int(rng.integers(0, min(8, len(arith))))]
        if arith and u < 0.75:
            return arith[int(rng.integers(0, len(arith)))]
        return leaves[int(rng.integers(0, len(leaves)))]

    while len(arith) < n_ops:
        op, a, b = int(rng.integers(3, 6)), pick(), pick()
        d = deg[a] + deg[b] if op == 5 else max(deg[a], deg[b])
        if d > max_degree:
            continue
        node = air._n(op, a, b)
        deg[node] = d
        arith.append(node)
    n_core = len(air.nodes)

    roots = [arith[int(rng.integers(0, n_ops))] for _ in range(n_defined)]
    whens = [0 if max(deg[r], 1) + 1 > max_degree else int(rng.integers(0, 4)) for r in roots]
    for j in rng.permutation(n_defined):
        j = int(j)
        air.assert_zero(air.sub(roots[j], air.local(n_inputs + j)), whens[j])

    t = rng.integers(0, P, size=(n, width), dtype=np.uint64)
    rows = [[int(x) for x in t[r]] for r in range(n)]
    for r in range(n):
        v = _eval_nodes(air.nodes, n_core, rows[r], rows[(r + 1) % n])
        for j in range(n_defined):
            if whens[j] == 0 or (whens[j] == 1 and r == 0) or (whens[j] == 2 and r == n - 1) or (whens[j] == 3 and r < n - 1):
                t[r, n_inputs + j] = v[roots[j]]
    return air, t


def live_chain(p25, m):
    """width 2, m + 1 values alive together: v0 = 3 x, v_{i+1} = v_i + x for m steps, total = v0 + v_m + v_{m-1} + ... + v_1
    (the first value of the chain is the first operand of the sum and every other one waits for its turn), and
    total * x = y on every row."""
    air = p25.Air(2)
    x = air.local(0)
    v = [air.mul(x, air.const(3))]
    for _ in range(m):
        v.append(air.add(v[-1], x))
    total = v[0]
    for u in reversed(v[1:]):
        total = air.add(total, u)
    air.assert_zero(air.sub(air.mul(total, x), air.local(1)))
    return air


def live_chain_trace(m, log_n, seed=1):
    rng = np.random.default_rng(seed)
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    k = sum(3 + i for i in range(m + 1))        # total = (sum of (3 + i)) x
    for r in range(1 << log_n):
        x = int(rng.integers(0, P, dtype=np.uint64))
        t[r] = (x, k * x % P * x % P)
    return t


def slot_churn(p25, steps=150, n_roots=70):
    """width 2, several hundred arithmetic nodes of which only a few are alive at any time: a program the device form
    holds ONLY if every slot goes back on its last use.  A chain acc <- acc + x | x + acc | acc * c | c * acc passes its
    value on as the left and as the right operand in turn (more than P3_MAX_LIVE times each), acc * x = y holds on every
    row, and n_roots further constraints (x + c_k) - (c_k + x), zero for every trace, each end in an arithmetic root
    that nothing reads again.  Returns (air, node of acc * x)."""
    air = p25.Air(2)
    x = air.local(0)
    acc = air.mul(x, air.const(3))
    for i in range(steps):
        c = air.const(i + 2)
        acc = (air.add(acc, x), air.add(x, acc), air.mul(acc, c), air.mul(c, acc))[i % 4]
    y = air.mul(acc, x)
    air.assert_zero(air.sub(y, air.local(1)))
    for k in range(n_roots):
        c = air.const(P - 1 - k)
        air.assert_zero(air.sub(air.add(x, c), air.add(c, x)), k % 4)
    return air, y


def slot_churn_trace(air, y_node, log_n, seed=1):
    rng = np.random.default_rng(seed)
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    for r in range(1 << log_n):
        x = int(rng.integers(0, P, dtype=np.uint64))
        t[r] = (x, _eval_nodes(air.nodes, y_node + 1, [x, 0], [0, 0])[y_node])
    return t


def constant_pair(p25, y0):
    """width 2, a trace that never moves: next x = x, next y = y^2, first row (p - 1, y0).  With y0 in {0, 1} the trace is
    (p - 1, y0) on every row: constant columns, a zero quotient, zero FRI layers when y0 = 0."""
    air = p25.Air(2)
    x, y = air.local(0), air.local(1)
    air.when_transition(air.sub(air.next(0), x))
    air.when_transition(air.sub(air.next(1), air.mul(y, y)))
    air.when_first_row(air.sub(x, air.const(P - 1)))
    air.when_first_row(air.sub(y, air.const(y0)))
    return air


def constant_pair_trace(y0, log_n):
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    t[:, 0], t[:, 1] = P - 1, y0
    return t


# The random_dag cases of the device prover's tests: every seed at every (max_degree, log_blowup) class; 3 queries, 4 PoW
# bits.  DAG_BAD_CELL is the cell the second proof of a case increments: row 5 of defined column 1.
DAG_SEEDS = tuple(range(12))
DAG_CLASSES = ((2, 1), (3, 1), (5, 2), (9, 3))
DAG_LOG_N, DAG_QUERIES, DAG_POW_BITS, DAG_BAD_CELL = 4, 3, 4, (5, 7)


def dag_case(p25, seed, max_degree):
    return random_dag(p25, seed, n_inputs=6, n_defined=10, n_ops=160, max_degree=max_degree, log_n=DAG_LOG_N)


def bump(trace, row, col):
    """A copy of `trace` with one cell incremented (mod p)."""
    t = trace.copy()
    t[row, col] = (int(t[row, col]) + 1) % P
    return t
