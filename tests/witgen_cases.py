"""One small circuit per witness-generator kind (blob kinds 0 to 20), built with tests/blob_writer.py, with a table of
boundary-valued operand rows and a model of the generator's outputs in plain Python integers.

In every circuit each dependency of the generator under test is a circuit input and every principal output is connected to
a further input (the "expectation"), so that a wrong output word is a copy-constraint conflict (status 4), not a silent
difference.  A row of a table is the operands; `Case.inputs(row)` appends the expectations the model computes.  The models are
written from the generators' definitions (upstream's gate files); they call neither the oracle nor
the library.  tests/test_witgen_cases_cpu.py holds the oracle's generators to them, tests/test_gpu_witgen_edge_values.py the
device's.

No circuit has more than 2^6 rows.
"""
import os
import re

import numpy as np

import blob_writer as bw
import edge_values as ev
from conftest import ROOT
from edge_values import EDGE, EPS, P

L = len(EDGE)
W = 7                                                 # F_p^2 = F_p[X] / (X^2 - 7)


# ---- F_p^2 in Python integers -------------------------------------------------------------------------------------------
def e_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def e_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def e_mul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def e_scale(x, s):
    return (x[0] * s % P, x[1] * s % P)


def e_inv(x):
    norm = (x[0] * x[0] - W * x[1] * x[1]) % P
    assert norm, "zero has no inverse"
    n = pow(norm, P - 2, P)
    return (x[0] * n % P, (P - x[1]) * n % P)


def pairs(flat):
    return [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]


# ---- operand tables -----------------------------------------------------------------------------------------------------
def edge_rows(k, i_range=None, j_range=None):
    """Rows of k operands from EDGE.  Operand m of row (i, j) is EDGE[(i A_m + j B_m) mod L] with (A_m, B_m) = (1, 0), (1, 1),
    (0, 1), (2, 3), (1, 2), (1, 3), ...  Two positions whose vectors have a determinant that is a unit mod L see EVERY ordered
    pair of EDGE over all (i, j): that holds for every pair among the first four positions but (2, 3) -- the multiplicands
    and the addend of an arithmetic op, and the four component products a0 b0, a1 b1, a0 b1, a1 b0 of an extension product
    (a0, a1) (b0, b1) -- and is asserted below."""
    coef = [(1, 0), (1, 1), (0, 1), (2, 3)] + [(1, s) for s in range(2, L)]
    out = []
    for i in (range(L) if i_range is None else i_range):
        for j in (range(L) if j_range is None else j_range):
            out.append([EDGE[(i * coef[m % len(coef)][0] + j * coef[m % len(coef)][1] + m // len(coef)) % L] for m in range(k)])
    return out


for _a, _b in ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3)):
    assert len({(r[_a], r[_b]) for r in edge_rows(4)}) == L * L


class Case:
    """name; the MiniCircuit and its blob; n_ops operands; `model(ops)` -> {target: value} for every modelled output; the
    principal outputs (connected to the expectation inputs, in input order); rows of operands; the generator kinds covered."""

    def __init__(self, name, circuit, n_ops, principal, model, rows, kinds, gates):
        self.name, self.circuit, self.n_ops, self.principal, self.model, self.rows = name, circuit, n_ops, principal, model, rows
        self.kinds, self.gates = set(kinds), set(gates)
        assert len(circuit.inputs) == n_ops
        for t in principal:
            circuit.connect(t, circuit.input())
        self.blob = circuit.to_blob()
        assert all(len(r) == n_ops for r in rows), name

    def inputs(self, ops):
        m = self.model(list(ops))
        return np.array([int(v) % P for v in ops] + [m[t] for t in self.principal], dtype=np.uint64)

    def wires(self, ops):
        """{(row, column): value} for the modelled outputs that are wires."""
        return {(t[1], t[2]): v for t, v in self.model(list(ops)).items() if t[0] == "w"}

    def wrong(self, ops, which=0):
        """The inputs of `ops` with one expectation off by one."""
        inp = self.inputs(ops)
        inp[self.n_ops + which] = (int(inp[self.n_ops + which]) + 1) % P
        return inp


CONSTS3 = (0, 1, P - 1)


# ---- kind 2 / 3 / 14: ArithmeticBase, MulExtension, ArithmeticExtension ------------------------------------------------------
def arithmetic_case(**config):
    c = bw.MiniCircuit(**config)
    a, b, d = c.input(), c.input(), c.input()
    outs = {(c0, c1): c.arithmetic(c0, c1, a, b, d) for c0 in CONSTS3 for c1 in CONSTS3}

    def model(ops):
        x, y, z = ops
        return {t: (c0 * x * y + c1 * z) % P for (c0, c1), t in outs.items()}

    return Case("arithmetic", c, 3, list(outs.values()), model, edge_rows(3), {bw.GEN_ARITHMETIC}, {bw.G_ARITHMETIC})


def mul_extension_case(**config):
    c = bw.MiniCircuit(**config)
    ins = [c.input() for _ in range(4)]
    outs = {c0: c.mul_extension(c0, ins[0:2], ins[2:4]) for c0 in CONSTS3}

    def model(ops):
        r = e_mul(tuple(ops[0:2]), tuple(ops[2:4]))
        m = {}
        for c0, t in outs.items():
            m[t[0]], m[t[1]] = e_scale(r, c0)
        return m

    return Case("mul_extension", c, 4, [t for o in outs.values() for t in o], model, edge_rows(4), {bw.GEN_MUL_EXT}, {bw.G_MUL_EXT})


def arithmetic_extension_case():
    c = bw.MiniCircuit()
    ins = [c.input() for _ in range(6)]
    outs = {(c0, c1): c.arithmetic_extension(c0, c1, ins[0:2], ins[2:4], ins[4:6]) for c0 in CONSTS3 for c1 in CONSTS3}

    def model(ops):
        r, ad = e_mul(tuple(ops[0:2]), tuple(ops[2:4])), tuple(ops[4:6])
        m = {}
        for (c0, c1), t in outs.items():
            m[t[0]], m[t[1]] = e_add(e_scale(r, c0), e_scale(ad, c1))
        return m

    return Case("arithmetic_extension", c, 6, [t for o in outs.values() for t in o], model, edge_rows(6), {bw.GEN_ARITH_EXT},
                {bw.G_ARITH_EXT})


# ---- kind 4: QuotientGeneratorExtension ------------------------------------------------------------------------------------
_Z = (3, 5)
NORM_ONE = e_mul(_Z, e_inv((_Z[0], P - _Z[1])))          # z / conj(z): norm 1, neither component 0
assert (NORM_ONE[0] ** 2 - W * NORM_ONE[1] ** 2) % P == 1 and NORM_ONE[1]
DENOMINATORS = [(1, 0), (0, 1), (P - 1, P - 1), NORM_ONE]


def quotient_extension_case(**config):
    c = bw.MiniCircuit(**config)
    ins = [c.input() for _ in range(4)]
    q = c.div_extension(ins[0:2], ins[2:4])

    def model(ops):
        den = tuple(ops[2:4])
        r = e_mul(tuple(ops[0:2]), e_inv(den)) if den != (0, 0) else (0, 0)      # den = 0: the zero-divisor rows only
        return {q[0]: r[0], q[1]: r[1]}

    # every ordered pair of EDGE as a numerator, the denominators in turn (row (i, j) takes number i + 2 j: each of the four
    # meets 100 numerators), then every denominator under the numerators (0, 0), (p - 1, p - 1) and itself
    rows = [num + list(DENOMINATORS[(k // L + 2 * (k % L)) % 4]) for k, num in enumerate(edge_rows(2))]
    rows += [list(num) + list(den) for den in DENOMINATORS for num in ((0, 0), (P - 1, P - 1), den)]
    return Case("quotient_extension", c, 4, list(q), model, rows, {bw.GEN_QUOTIENT_EXT, bw.GEN_MUL_EXT}, {bw.G_MUL_EXT})


# rows outside the table (test 4e): upstream panics on them
QUOTIENT_ZERO_DIVISOR = {"num != 0": [EPS, P - 1, 0, 0], "num == 0": [0, 0, 0, 0]}


# ---- kinds 5 to 8: BaseSplit, WireSplit, BaseSum, LowHigh ----------------------------------------------------------------
SPLIT_X = [0, 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, P - 1, 0xFFFFFFFF00000000]
SPLIT_N = [1, 31, 32, 33, 63]
assert 0xFFFFFFFF00000000 == P - 1                    # the issue lists it under both names; one row each all the same


def low_high_case(**config):
    """x -> (x mod 2^n, x >> n) for every n of SPLIT_N (what the shifts are made of), each half range-checked on a BaseSum
    row whose BaseSplitGenerator writes its bits."""
    c = bw.MiniCircuit(**config)
    x = c.input()
    halves, bits = {}, {}
    for n in SPLIT_N:
        before = len(c.rows)
        halves[n] = c.split_low_high(x, n)
        bits[n] = ([("w", before, 1 + k) for k in range(n)], [("w", before + 1, 1 + k) for k in range(64 - n)])
        assert c.rows[before][0] == bw.G_BASE_SUM and c.rows[before + 1][0] == bw.G_BASE_SUM

    def model(ops):
        v, m = ops[0], {}
        for n in SPLIT_N:
            low, high = v % (1 << n), v >> n
            m[halves[n][0]], m[halves[n][1]] = low, high
            for k, t in enumerate(bits[n][0]):
                m[t] = (low >> k) & 1
            for k, t in enumerate(bits[n][1]):
                m[t] = (high >> k) & 1
            m[("w", bits[n][0][0][1], 0)], m[("w", bits[n][1][0][1], 0)] = low, high        # the rows' sum wires
        return m

    return Case("low_high", c, 1, [t for n in SPLIT_N for t in halves[n]], model, [[v] for v in SPLIT_X],
                {bw.GEN_LOW_HIGH, bw.GEN_BASE_SPLIT, bw.GEN_ARITHMETIC}, {bw.G_BASE_SUM, bw.G_ARITHMETIC})


def reverse_bits_case():
    """x -> its 64 bits (split_le: WireSplit + BaseSplit) -> for every n of SPLIT_N the low n bits reversed (le_sum:
    BaseSumGenerator), the shape of reverse_bits_len."""
    c = bw.MiniCircuit()
    x = c.input()
    first = len(c.rows)
    bits = c.split_le_64(x)
    sums = {n: c.le_sum(bits[:n][::-1]) for n in SPLIT_N}

    def model(ops):
        v = ops[0]
        m = {t: (v >> k) & 1 for k, t in enumerate(bits)}
        m[("w", first, 0)], m[("w", first + 1, 0)] = v % (1 << 63), v >> 63
        for n in SPLIT_N:
            m[sums[n]] = sum(((v >> k) & 1) << (n - 1 - k) for k in range(n))
        return m

    return Case("reverse_bits", c, 1, [sums[n] for n in SPLIT_N], model, [[v] for v in SPLIT_X],
                {bw.GEN_WIRE_SPLIT, bw.GEN_BASE_SPLIT, bw.GEN_BASE_SUM, bw.GEN_ARITHMETIC}, {bw.G_BASE_SUM, bw.G_ARITHMETIC})


# ---- kind 9: Exponentiation ---------------------------------------------------------------------------------------------
EXP_BASES = [0, 1, P - 1, 7, ev.TWO_ADIC]
assert pow(ev.TWO_ADIC, 1 << 32, P) == 1 and pow(ev.TWO_ADIC, 1 << 31, P) != 1        # order exactly 2^32
EXP_BITS = {"all zero": [0] * 66, "all one": [1] * 66, "one-hot low": [1] + [0] * 65, "one-hot high": [0] * 65 + [1]}


def exponentiation_case():
    c = bw.MiniCircuit()
    base = c.input()
    bits = [c.input() for _ in range(bw.EXP_BITS)]
    out, inter = c.exponentiation(base, bits)

    def model(ops):
        b, e = ops[0], ops[1:]
        m = {}
        for i, t in enumerate(inter):                  # after the i + 1 most significant bits
            m[t] = pow(b, sum(e[65 - k] << (i - k) for k in range(i + 1)), P)
        m[out] = pow(b, sum(bit << k for k, bit in enumerate(e)), P)
        return m

    rows = [[b] + e for b in EXP_BASES for e in EXP_BITS.values()]
    return Case("exponentiation", c, 1 + bw.EXP_BITS, [out], model, rows, {bw.GEN_EXPONENTIATION}, {bw.G_EXPONENTIATION})


# ---- kind 11: U32Arithmetic ---------------------------------------------------------------------------------------------
M32 = (1 << 32) - 1
# "All 32 two-bit limbs 3" is the word 2^64 - 1.  It is no field element, and u32 operands reach x y + z = p - 1 at the
# most, so no row can hold it.  The row kept in its place has the most limbs of 3 a generator can emit: x y + z =
# 0xFFFFFFFEFFFFFFFF (the largest word below the high == 2^32 - 1 branch), 31 limbs of 3 and the lowest limb of `high` 2.
ALL_BUT_ONE_LIMB_3 = [M32, M32, M32 - 1]               # (2^32 - 1)^2 + 2^32 - 2
assert ALL_BUT_ONE_LIMB_3[0] * ALL_BUT_ONE_LIMB_3[1] + ALL_BUT_ONE_LIMB_3[2] == 0xFFFFFFFEFFFFFFFF
U32_TRIPLES = [[M32, M32, M32],                       # x y + z = p - 1: high = 2^32 - 1, low = 0, the diff == 0 branch
               [0, 0, 0], [M32, M32, 0], [1 << 16, 1 << 16, M32], ALL_BUT_ONE_LIMB_3]


def u32_arithmetic_model(x, y, z):
    """(low, high, inverse, limbs): the reference generator computes x y + z IN THE FIELD and splits the canonical word;
    inverse = 1 / (2^32 - 1 - high), or 0 where that difference is 0."""
    o = (x * y + z) % P
    low, high = o & M32, o >> 32
    diff = (M32 - high) % P
    return low, high, (pow(diff, P - 2, P) if diff else 0), [(o >> (2 * j)) & 3 for j in range(32)]


def u32_arithmetic_case():
    c = bw.MiniCircuit()
    ins = [c.input() for _ in range(9)]
    ops_out = [c.mul_add_u32(*ins[3 * i:3 * i + 3]) for i in range(3)]
    row = ops_out[0][0][1]

    def model(ops):
        m = {}
        for i in range(3):
            low, high, inv, limbs = u32_arithmetic_model(*ops[3 * i:3 * i + 3])
            m[ops_out[i][0]], m[ops_out[i][1]], m[("w", row, 6 * i + 5)] = low, high, inv
            for j, v in enumerate(limbs):
                m[("w", row, 18 + 32 * i + j)] = v
        return m

    n = len(U32_TRIPLES)
    rows = [U32_TRIPLES[r] + U32_TRIPLES[(r + 1) % n] + U32_TRIPLES[(r + 2) % n] for r in range(n)]
    return Case("u32_arithmetic", c, 9, [t for o in ops_out for t in o], model, rows, {bw.GEN_U32_ARITHMETIC}, {bw.G_U32_ARITHMETIC})


# ---- kinds 12, 13: U32Interleave, UninterleaveToU32 ---------------------------------------------------------------------------
INTERLEAVE_X = [0, 1, 0x80000000, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF]
UNINTERLEAVE_X = INTERLEAVE_X + [0xF555555555555555, (1 << 64) - (1 << 32)]
assert UNINTERLEAVE_X[-1] == P - 1


def u32_bits_case():
    c = bw.MiniCircuit()
    xs = [c.input() for _ in range(3)]
    ys = [c.input() for _ in range(2)]
    il = [c.interleave_u32(x) for x in xs]
    un = [c.uninterleave_to_u32(y) for y in ys]
    il_row, un_row = il[0][1], un[0][0][1]

    def model(ops):
        m = {}
        for i, x in enumerate(ops[:3]):                # 32 bits, most significant first; bit k of x goes to bit 2k
            for b in range(32):
                m[("w", il_row, 6 + 32 * i + b)] = (x >> (31 - b)) & 1
            m[il[i]] = sum(((x >> k) & 1) << (2 * k) for k in range(32))
        for i, y in enumerate(ops[3:]):                # 64 bits, most significant first; evens = bits 0, 2, .. of that order
            be = [(y >> (63 - b)) & 1 for b in range(64)]
            for b in range(64):
                m[("w", un_row, 6 + 64 * i + b)] = be[b]
            m[un[i][0]] = sum(be[2 * j] << (31 - j) for j in range(32))
            m[un[i][1]] = sum(be[2 * j + 1] << (31 - j) for j in range(32))
        return m

    ni, nu = len(INTERLEAVE_X), len(UNINTERLEAVE_X)
    rows = [[INTERLEAVE_X[(r + k) % ni] for k in range(3)] + [UNINTERLEAVE_X[(r + 3 * k) % nu] for k in range(2)] for r in range(nu)]
    return Case("u32_bits", c, 5, il + [t for u in un for t in u], model, rows, {bw.GEN_U32_INTERLEAVE, bw.GEN_U32_UNINTERLEAVE},
                {bw.G_U32_INTERLEAVE, bw.G_U32_UNINTERLEAVE})


# ---- kinds 10, 15: Poseidon2, Poseidon ------------------------------------------------------------------------------------
def _words(path, name=None):
    src = open(os.path.join(ROOT, "plonky2.5_amd", "csrc", path)).read()
    if name is not None:
        src = re.search(r"%s\[\d+\]\s*=\s*\{([^}]*)\}" % name, src).group(1)
    return [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)ULL", src)]


POSEIDON_RC = _words("poseidon_constants.inc")
P2_RC, P2_RC_MID, P2_DIAG_M1 = (_words("poseidon2_constants.inc", n) for n in ("P2_RC", "P2_RC_MID", "P2_MAT_DIAG_M_1"))
assert (len(POSEIDON_RC), len(P2_RC), len(P2_RC_MID), len(P2_DIAG_M1)) == (360, 96, 22, 12)
MDS_CIRC, MDS_DIAG0 = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20], 8


def mds_layer(s):
    """Poseidon's MDS matrix circ(MDS_CIRC) + diag(8, 0, ..): out_r = sum_i circ_i s_(i + r) + 8 s_0 [r = 0]."""
    return [(sum(MDS_CIRC[i] * s[(i + r) % 12] for i in range(12)) + (MDS_DIAG0 * s[0] if r == 0 else 0)) % P for r in range(12)]


def poseidon_trace(state):
    """(106 S-box inputs in round order, final state): 4 full rounds, 22 partial, 4 full; the S-box inputs of round 0 are the
    gate's own inputs and are not recorded."""
    s, tr = list(state), []
    for r in range(30):
        s = [(v + POSEIDON_RC[12 * r + i]) % P for i, v in enumerate(s)]
        if r < 4 or r >= 26:
            if r:
                tr += s
            s = [pow(v, 7, P) for v in s]
        else:
            tr.append(s[0])
            s[0] = pow(s[0], 7, P)
        s = mds_layer(s)
    return tr, s


M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]          # the 4 x 4 MDS block of the Poseidon2 paper


def p2_external(s):
    """Poseidon2's external layer for width 12: M4 on each block of four, then every word plus the sum of the three blocks'
    words at its position (circ(2 M4, M4, M4))."""
    y = []
    for b in range(3):
        x = s[4 * b:4 * b + 4]
        y += [sum(M4[r][k] * x[k] for k in range(4)) % P for r in range(4)]
    col = [(y[k] + y[4 + k] + y[8 + k]) % P for k in range(4)]
    return [(y[i] + col[i % 4]) % P for i in range(12)]


def p2_internal(s):
    """1 1^T + diag(mu - 1): every word times its diagonal entry less one, plus the sum of all."""
    tot = sum(s) % P
    return [(v * (P2_DIAG_M1[i] - 1) + tot) % P for i, v in enumerate(s)]


def poseidon2_trace(state):
    s, tr = p2_external(list(state)), []
    for r in range(4):
        s = [(v + P2_RC[12 * r + i]) % P for i, v in enumerate(s)]
        if r:
            tr += s
        s = p2_external([pow(v, 7, P) for v in s])
    for r in range(22):
        s[0] = (s[0] + P2_RC_MID[r]) % P
        tr.append(s[0])
        s[0] = pow(s[0], 7, P)
        s = p2_internal(s)
    for r in range(4, 8):
        s = [(v + P2_RC[12 * r + i]) % P for i, v in enumerate(s)]
        tr += s
        s = p2_external([pow(v, 7, P) for v in s])
    return tr, s


PERM_STATES = {"all 0": [0] * 12, "all p-1": [P - 1] * 12}
PERM_STATES.update({f"edge({s})": [int(v) for v in ev.edge(12, s)] for s in (1, 2, 3)})


def permutation_case(kinds, name, swaps):
    """One row per gate kind of `kinds` (bw.G_POSEIDON2 / bw.G_POSEIDON), every one reading 12 inputs and a swap input of
    its own directly: the generators all sit in the first level.  Operands: per row 12 state words, then the swap."""
    c = bw.MiniCircuit()
    ins = [[c.input() for _ in range(13)] for _ in kinds]
    rows_of = [(c.poseidon2_row if k == bw.G_POSEIDON2 else c.poseidon_row)(i[:12], i[12]) for k, i in zip(kinds, ins)]

    def model(ops):
        m = {}
        for n, (k, row) in enumerate(zip(kinds, rows_of)):
            st, swap = ops[13 * n:13 * n + 12], ops[13 * n + 12]
            for i in range(4):                         # delta_i = swap (b_i - a_i); the halves are exchanged for swap == 1 only
                m[("w", row, 25 + i)] = swap * (st[4 + i] - st[i]) % P
            if swap == 1:
                st = st[4:8] + st[0:4] + st[8:12]
            tr, out = (poseidon2_trace if k == bw.G_POSEIDON2 else poseidon_trace)(st)
            for i, v in enumerate(tr):
                m[("w", row, 29 + i)] = v
            for i, v in enumerate(out):
                m[("w", row, 12 + i)] = v
        return m

    # the swaps alternate from row to row, an exchange first, so that a batch of one or two rows has one too
    names = list(PERM_STATES)
    rows = []
    for s in range(len(names)):
        for r, sw in enumerate(swaps):
            rows.append([w for n in range(len(kinds)) for w in PERM_STATES[names[(s + 2 * n + r) % len(names)]] + [sw[n]]])
    gk = {bw.G_POSEIDON2: bw.GEN_POSEIDON2, bw.G_POSEIDON: bw.GEN_POSEIDON}
    return Case(name, c, 13 * len(kinds), [("w", row, 12 + i) for row in rows_of for i in range(12)], model, rows,
                {gk[k] for k in kinds}, set(kinds))


def poseidon2_case():
    return permutation_case([bw.G_POSEIDON2], "poseidon2", [(1,), (0,)])


def poseidon_case():
    return permutation_case([bw.G_POSEIDON], "poseidon", [(1,), (0,)])


def mixed_poseidon_case():
    """A Poseidon2 and a Poseidon generator in ONE level: DeviceCircuit makes the level cooperative for Poseidon2, and the
    Poseidon generator runs in the per-lane `case GEN_POSEIDON` body of witgen_level_body."""
    return permutation_case([bw.G_POSEIDON2, bw.G_POSEIDON], "mixed_poseidon", [(1, 1), (0, 1), (1, 0), (0, 0)])


def mixed_swap_rows(swap):
    """Mixed-level rows with `swap` (2, p - 1: not boolean) on either kind, 0 on the other."""
    st = PERM_STATES["edge(1)"], PERM_STATES["all p-1"]
    return [st[0] + [swap] + st[1] + [0], st[1] + [0] + st[0] + [swap]]


# ---- kind 20: PoseidonMds -------------------------------------------------------------------------------------------------
def poseidon_mds_case():
    c = bw.MiniCircuit()
    ins = [c.input() for _ in range(24)]
    outs = c.poseidon_mds(pairs(ins))

    def model(ops):
        m = {}
        for comp in range(2):                          # the layer acts on the two components of the 12 pairs separately
            o = mds_layer([ops[2 * i + comp] for i in range(12)])
            for r in range(12):
                m[outs[2 * r + comp]] = o[r]
        return m

    rows = edge_rows(24, j_range=(0, 11)) + [[P - 1] * 24, [0] * 24]
    return Case("poseidon_mds", c, 24, outs, model, rows, {bw.GEN_POSEIDON_MDS}, {bw.G_POSEIDON_MDS})


# ---- kind 16: RandomAccess ------------------------------------------------------------------------------------------------
RA_EXTRA = (EPS, P - 1)


def random_access_case():
    c = bw.MiniCircuit()
    ins = [[c.input() for _ in range(17)] for _ in range(4)]
    claimed = [c.random_access(i[0], i[1:], RA_EXTRA) for i in ins]
    row = claimed[0][1]
    assert all(t[1] == row for t in claimed)           # the four copies of ONE row

    def model(ops):
        m = {("w", row, 72): RA_EXTRA[0], ("w", row, 73): RA_EXTRA[1]}
        for cp in range(4):
            idx, items = ops[17 * cp], ops[17 * cp + 1:17 * cp + 17]
            m[claimed[cp]] = items[idx]
            for k in range(4):
                m[("w", row, 74 + 4 * cp + k)] = (idx >> k) & 1
        return m

    rows = [[w for cp in range(4) for w in [(r + 5 * cp) % 16] + [EDGE[(r + 3 * cp + k) % L] for k in range(16)]] for r in range(16)]
    return Case("random_access", c, 68, claimed, model, rows, {bw.GEN_RANDOM_ACCESS, bw.GEN_CONSTANT}, {bw.G_RANDOM_ACCESS})


def random_access_bad_index_row(case, index):
    """A row of the table with copy 2's index replaced (16, p - 1: outside the list)."""
    ops = list(case.rows[3])
    ops[17 * 2] = index
    return ops


# ---- kinds 17, 18: Reducing, ReducingExtension --------------------------------------------------------------------------
ALPHAS = [(0, 0), (1, 0), (P - 1, P - 1), (0, 1)]


def reducing_case(ext, **config):
    n = bw.REDX_COEFFS if ext else bw.RED_COEFFS
    c = bw.MiniCircuit(**config)
    alpha, old = [c.input(), c.input()], [c.input(), c.input()]
    co = [c.input() for _ in range(2 * n if ext else n)]
    out, accs = c.reducing(alpha, old, pairs(co) if ext else co, ext)

    def model(ops):
        al, acc = tuple(ops[0:2]), tuple(ops[2:4])
        cs = pairs(ops[4:]) if ext else [(v, 0) for v in ops[4:]]
        m = {}
        for i, cf in enumerate(cs):                    # acc <- acc alpha + coefficient; every accumulator has its wires
            acc = e_add(e_mul(acc, al), cf)
            m[accs[2 * i]], m[accs[2 * i + 1]] = acc
        return m

    nco = len(co)
    coeff_sets = [[P - 1] * nco, [EDGE[k % L] for k in range(nco)], [0] * nco, [EDGE[(5 * k + 3) % L] for k in range(nco)]]
    rows = [list(al) + [EDGE[(3 * a + 7 * s) % L], EDGE[(5 * a + 11 * s + 1) % L]] + cs
            for a, al in enumerate(ALPHAS) for s, cs in enumerate(coeff_sets)]
    return Case("reducing_extension" if ext else "reducing", c, 4 + nco, list(out), model, rows,
                {bw.GEN_REDUCING_EXT if ext else bw.GEN_REDUCING}, {bw.G_REDUCING_EXT if ext else bw.G_REDUCING})


# ---- kind 19: CosetInterpolation -------------------------------------------------------------------------------------------
G16 = ev.root_of_unity(4)
CI_SHIFTS = [1, 7, P - 1]
CI_CHUNKS = (6, 11, 16)                                # points consumed after each of the gate's three steps (degree 6)


def coset_interpolation_model(shift, values, point):
    """x = point / shift; the value at x of the polynomial of degree < 16 through (g^i, values[i]), by Lagrange's formula;
    and the two intermediate states of the gate's recurrence written as the sums they stand for: after k points,
    eval_k = sum_(i<k) (g^i / 16) v_i prod_(j<k, j != i) (x - g^j) and prod_k = prod_(j<k) (x - g^j)."""
    x = e_scale(point, pow(shift, P - 2, P))           # shift = 0 (the zero-divisor row only): 0^(p-2) = 0, so x = 0
    xs = [pow(G16, i, P) for i in range(16)]
    inv16 = pow(16, P - 2, P)

    def state(k):
        ev_k, pr_k = (0, 0), (1, 0)
        for j in range(k):
            pr_k = e_mul(pr_k, e_sub(x, (xs[j], 0)))
        for i in range(k):
            t = e_scale(values[i], xs[i] * inv16 % P)
            for j in range(k):
                if j != i:
                    t = e_mul(t, e_sub(x, (xs[j], 0)))
            ev_k = e_add(ev_k, t)
        return ev_k, pr_k

    value = (0, 0)
    for i in range(16):
        t = values[i]
        for j in range(16):
            if j != i:
                t = e_scale(e_mul(t, e_sub(x, (xs[j], 0))), pow((xs[i] - xs[j]) % P, P - 2, P))
        value = e_add(value, t)
    return x, state(CI_CHUNKS[0]), state(CI_CHUNKS[1]), value


def coset_interpolation_case():
    c = bw.MiniCircuit()
    shift = c.input()
    vals = [c.input() for _ in range(32)]
    point = [c.input(), c.input()]
    value, outs = c.coset_interpolation(shift, pairs(vals), point)

    def model(ops):
        x, (e1, p1), (e2, p2), v = coset_interpolation_model(ops[0], pairs(ops[1:33]), tuple(ops[33:35]))
        return dict(zip(outs, list(x) + list(e1) + list(p1) + list(e2) + list(p2) + list(v)))

    value_sets = [[EDGE[(k + 2) % L] for k in range(32)], [EDGE[(7 * k + 5) % L] for k in range(32)]]
    rows = []
    for s, sh in enumerate(CI_SHIFTS):
        points = [(sh * pow(G16, k, P) % P, 0) for k in (0, 5, 6, 10, 11, 15)]       # domain points: one `term` is zero
        points += [(EDGE[(s + 9) % L], 0), (EDGE[(s + 14) % L], EDGE[(s + 18) % L])]  # a base-field point, an extension point
        for k, pt in enumerate(points):
            rows.append([sh] + value_sets[(k + s) % 2] + list(pt))
    return Case("coset_interpolation", c, 35, list(value), model, rows, {bw.GEN_COSET_INTERP}, {bw.G_COSET_INTERP})


def coset_zero_shift_row(case):
    """A row of the table (an extension point) with the shift replaced by 0: upstream panics on it."""
    ops = list(case.rows[7])
    ops[0] = 0
    return ops


# ---- the list ------------------------------------------------------------------------------------------------------------
BUILDERS = [arithmetic_case, mul_extension_case, arithmetic_extension_case, quotient_extension_case, low_high_case,
            reverse_bits_case, exponentiation_case, u32_arithmetic_case, u32_bits_case, poseidon2_case, poseidon_case,
            mixed_poseidon_case, poseidon_mds_case, random_access_case, lambda **config: reducing_case(False, **config), lambda **config: reducing_case(True, **config),
            coset_interpolation_case]
_cache = {}


def all_cases():
    """name -> Case, built once a process."""
    if not _cache:
        for b in BUILDERS:
            case = b()
            _cache[case.name] = case
    return _cache


NAMES = ["arithmetic", "mul_extension", "arithmetic_extension", "quotient_extension", "low_high", "reverse_bits", "exponentiation",
         "u32_arithmetic", "u32_bits", "poseidon2", "poseidon", "mixed_poseidon", "poseidon_mds", "random_access", "reducing",
         "reducing_extension", "coset_interpolation"]
# the circuits whose batch forms are tested in full (permutation generators: the cooperative form; U32Arithmetic: per lane)
FULL_BATCH = ["poseidon2", "poseidon", "mixed_poseidon", "u32_arithmetic"]


def generator_kinds(blob):
    """The generator kinds of a blob's generator table, read with the layout of INTEGRATION.md section 5 alone."""
    import struct
    h = struct.unpack_from("<32Q", blob, 8)
    n = 1 << h[0]
    pad = lambda k: (k + 1) // 2 * 8
    off = 8 + 256 + 32 * h[14] + 8 * h[10] + pad(n) + 8 * h[19] * n + 8 * h[2] + pad(h[17]) + pad(n * h[1] + h[16])
    out = []
    for _ in range(h[18]):
        kind, _c0, _c1, _aux, nd, no = struct.unpack_from("<6Q", blob, off)
        args = struct.unpack_from(f"<{nd + no}I", blob, off + 48)
        out.append((kind, args[:nd], args[nd:]))
        off += 48 + pad(nd + no)
    assert off == len(blob)
    return out


def blob_tables(blob):
    """(input target indices, representative map) of a blob."""
    import struct
    h = struct.unpack_from("<32Q", blob, 8)
    n = 1 << h[0]
    pad = lambda k: (k + 1) // 2 * 8
    off = 8 + 256 + 32 * h[14] + 8 * h[10] + pad(n) + 8 * h[19] * n + 8 * h[2]
    inputs = struct.unpack_from(f"<{h[17]}I", blob, off)
    rep = struct.unpack_from(f"<{n * h[1] + h[16]}I", blob, off + pad(h[17]))
    return inputs, rep
