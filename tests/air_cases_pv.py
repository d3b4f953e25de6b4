"""AIRs with public values (p25_air.n_public, node op PUBLIC; include/p25.h) and their traces.

fib_pv      plonky3's own Fibonacci example with `pis = [a, b, x]`: the reference's FibonacciAir (src/p3/mod.rs:176-221) with
            its boundary constants replaced by public values -- first row a = pv0, b = pv1; last row c = pv2.
pv_mix(m)   width 2, m public values, every one of them in a constraint under its own weight, so that a wrong index or a
            wrong row offset into a batch's public values cannot cancel."""
import numpy as np

P = 0xFFFFFFFF00000001


def fib_pv(p25):
    air = p25.Air(3, n_public=3)
    la, lb, lc = air.local(0), air.local(1), air.local(2)
    na, nb = air.next(0), air.next(1)
    air.assert_zero(air.sub(air.add(la, lb), lc))
    air.when_first_row(air.sub(air.public(0), la))
    air.when_first_row(air.sub(air.public(1), lb))
    air.when_transition(air.sub(na, lb))
    air.when_transition(air.sub(nb, lc))
    air.when_last_row(air.sub(air.public(2), lc))
    return air


def fib_pv_trace(log_n, a, b):
    """-> (trace uint64[2^log_n][3], public values [a, b, x]) with x the last row's c."""
    n = 1 << log_n
    t = np.zeros((n, 3), dtype=np.uint64)
    a, b = int(a) % P, int(b) % P
    pv = [a, b, 0]
    for i in range(n):
        c = (a + b) % P
        t[i] = (a, b, c)
        a, b = b, c
    pv[2] = int(t[n - 1, 2])
    return t, np.array(pv, dtype=np.uint64)


def mix_weights(m):
    """The weights c_i of pv_mix(m): constants below p, no two alike."""
    w = [(0x9E3779B97F4A7C15 * (i + 1) + 2 * i + 1) % P for i in range(m)]
    assert len(set(w)) == m and 0 not in w
    return w


def pv_mix(p25, m):
    """Column 0 is constant along the trace (transition next0 = local0); first row local0 = sum c_i pv_i; every row
    local1 = local0^2 + pv_{m-1}."""
    air = p25.Air(2, n_public=m)
    x, y = air.local(0), air.local(1)
    air.when_transition(air.sub(air.next(0), x))
    acc = None
    for i, c in enumerate(mix_weights(m)):
        term = air.mul(air.const(c), air.public(i))
        acc = term if acc is None else air.add(acc, term)
    air.when_first_row(air.sub(x, acc))
    air.assert_zero(air.sub(y, air.add(air.mul(x, x), air.public(m - 1))))
    return air


def pv_mix_values(m, seed):
    rng = np.random.default_rng(1000 * m + seed)
    return rng.integers(0, P, size=m, dtype=np.uint64)


def pv_mix_trace(log_n, pv):
    pv = [int(v) for v in pv]
    x = sum(c * v for c, v in zip(mix_weights(len(pv)), pv)) % P
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    t[:, 0] = x
    t[:, 1] = (x * x + pv[-1]) % P
    return t
