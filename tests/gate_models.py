"""The constraints of every gate kind of the circuit blob (kinds 0 to 17) in plain Python, over a field handed in as a small
namespace: `Base` (integers mod p) for the prover's quotient, `Ext` (pairs in F_p[X] / (X^2 - 7)) for the verifier's identity
at zeta.

Written from the gates' definitions -- INTEGRATION.md section 5, upstream's gate files, and for the reference's own four
gates their `eval_unfiltered` -- as mathematics: sums with explicit weights where the definition is a sum, closed forms
where it is a recurrence.  They call neither the oracle nor the library and share no code with either's evaluators.
tests/test_quotient_model_cpu.py holds the oracle's evaluators to them, tests/test_gpu_quotient_model.py the device's.

`constraints(kind, F, wires, k0, k1, pi_hash)` -> the list of constraint values of one row, GATE_CONSTRAINTS[kind] long, in
the gate's own order.  `wires` are elements of F; k0, k1 (the row's constants) and the four words of pi_hash too.
`reads(kind)` -> what that list depends on.

Wire pairs (a, b) of the extension gates stand for a + b X in the algebra A = F[X] / (X^2 - 7) over whatever F is.
"""
import blob_writer as bw
from witgen_cases import M4, MDS_CIRC, MDS_DIAG0, P2_DIAG_M1, P2_RC, P2_RC_MID, POSEIDON_RC

P = bw.P
W = 7


class Base:
    """F_p in Python integers."""
    zero, one = 0, 1

    @staticmethod
    def k(v):
        return v % P

    @staticmethod
    def add(x, y):
        return (x + y) % P

    @staticmethod
    def sub(x, y):
        return (x - y) % P

    @staticmethod
    def mul(x, y):
        return x * y % P

    @staticmethod
    def scale(x, s):
        return x * s % P

    @staticmethod
    def lin(coeffs, xs):
        """sum_i coeffs[i] xs[i], the coefficients integers."""
        return sum(c * x for c, x in zip(coeffs, xs)) % P


class Ext:
    """F_p^2 = F_p[X] / (X^2 - 7) in pairs of Python integers."""
    zero, one = (0, 0), (1, 0)

    @staticmethod
    def k(v):
        return (v % P, 0)

    @staticmethod
    def add(x, y):
        return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)

    @staticmethod
    def sub(x, y):
        return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)

    @staticmethod
    def mul(x, y):
        return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)

    @staticmethod
    def scale(x, s):
        return (x[0] * s % P, x[1] * s % P)

    @staticmethod
    def lin(coeffs, xs):
        return (sum(c * x[0] for c, x in zip(coeffs, xs)) % P, sum(c * x[1] for c, x in zip(coeffs, xs)) % P)


# ---- helpers over any F ---------------------------------------------------------------------------------------------------
def _prod(F, xs):
    out = F.one
    for x in xs:
        out = F.mul(out, x)
    return out


def _in_range(F, x, bound):
    """x (x - 1) .. (x - (bound - 1)): zero exactly on 0 .. bound - 1."""
    return _prod(F, [F.sub(x, F.k(v)) for v in range(bound)])


def _pow7(F, x):
    x2 = F.mul(x, x)
    x3 = F.mul(x2, x)
    return F.mul(F.mul(x3, x3), x)


def _alg_mul(F, x, y):
    """(x0 + x1 X) (y0 + y1 X) in A."""
    return (F.add(F.mul(x[0], y[0]), F.scale(F.mul(x[1], y[1]), W)), F.add(F.mul(x[0], y[1]), F.mul(x[1], y[0])))


def _alg_add(F, x, y):
    return (F.add(x[0], y[0]), F.add(x[1], y[1]))


def _alg_sub(F, x, y):
    return (F.sub(x[0], y[0]), F.sub(x[1], y[1]))


def _alg_scale(F, x, s):
    """An element of A times an element of F."""
    return (F.mul(x[0], s), F.mul(x[1], s))


def _pair(w, i):
    return (w[i], w[i + 1])


# ---- the gates --------------------------------------------------------------------------------------------------------------
def _noop(F, w, k0, k1, pih):
    return []


def _constant(F, w, k0, k1, pih):
    """ConstantGate { num_consts: 2 }: constant i is what wire i holds."""
    return [F.sub(k, w[i]) for i, k in enumerate((k0, k1))]


def _public_input(F, w, k0, k1, pih):
    """PublicInputGate: wires 0..3 are the hash of the public inputs."""
    return [F.sub(w[i], pih[i]) for i in range(4)]


def _base_sum(F, w, k0, k1, pih):
    """BaseSumGate<2>, 63 limbs: sum_i 2^i limb_i is wire 0; every limb is a bit."""
    limbs = [w[1 + i] for i in range(bw.BASE_SUM_LIMBS)]
    return [F.sub(F.lin([1 << i for i in range(bw.BASE_SUM_LIMBS)], limbs), w[0])] + [_in_range(F, b, 2) for b in limbs]


def _arithmetic(F, w, k0, k1, pih):
    """ArithmeticGate, 20 ops of (m0, m1, addend, out): out = k0 m0 m1 + k1 addend."""
    return [F.sub(w[4 * i + 3], F.add(F.mul(k0, F.mul(w[4 * i], w[4 * i + 1])), F.mul(k1, w[4 * i + 2]))) for i in range(bw.ARITH_OPS)]


def _mul_ext(F, w, k0, k1, pih):
    """MulExtensionGate, 13 ops of three pairs (a, b, out): out = k0 a b in A."""
    out = []
    for i in range(bw.EXT_OPS[bw.G_MUL_EXT][0]):
        a, b, o = (_pair(w, 6 * i + 2 * t) for t in range(3))
        out += list(_alg_sub(F, o, _alg_scale(F, _alg_mul(F, a, b), k0)))
    return out


def _arith_ext(F, w, k0, k1, pih):
    """ArithmeticExtensionGate, 10 ops of four pairs (m0, m1, addend, out): out = k0 m0 m1 + k1 addend in A."""
    out = []
    for i in range(bw.EXT_OPS[bw.G_ARITH_EXT][0]):
        m0, m1, ad, o = (_pair(w, 8 * i + 2 * t) for t in range(4))
        out += list(_alg_sub(F, o, _alg_add(F, _alg_scale(F, _alg_mul(F, m0, m1), k0), _alg_scale(F, ad, k1))))
    return out


def _exponentiation(F, w, k0, k1, pih):
    """ExponentiationGate, 66 bits: wire 0 the base, 1..66 the exponent's bits (little-endian), 67 the output, 68..133 the
    value after each bit, most significant first: v_i = v_(i-1)^2 (bit base + 1 - bit), v_(-1) = 1."""
    n = bw.EXP_BITS
    out = []
    for i in range(n):
        bit = w[1 + (n - 1 - i)]
        square = F.one if i == 0 else F.mul(w[68 + i - 1], w[68 + i - 1])
        factor = F.add(F.mul(bit, w[0]), F.sub(F.one, bit))
        out.append(F.sub(F.mul(square, factor), w[68 + i]))
    return out + [F.sub(w[67], w[68 + n - 1])]


def _u32_arithmetic(F, w, k0, k1, pih):
    """U32ArithmeticGate, 3 ops: (m0, m1, addend, low, high, inverse) at 6i, 32 two-bit limbs at 18 + 32i.  Per op: the
    canonicity check (inverse (2^32 - 1 - high) - 1) low; 2^32 high + low = m0 m1 + addend; the limbs' range checks from limb
    31 down to limb 0; the low 16 limbs are `low`, the high 16 `high`."""
    out = []
    for i in range(bw.MULTI_OPS[bw.G_U32_ARITHMETIC]):
        m0, m1, ad, low, high, inv = (w[6 * i + t] for t in range(6))
        limbs = [w[18 + 32 * i + j] for j in range(32)]
        not_max = F.sub(F.mul(inv, F.sub(F.k(0xFFFFFFFF), high)), F.one)
        out.append(F.mul(not_max, low))
        out.append(F.sub(F.add(F.scale(high, 1 << 32), low), F.add(F.mul(m0, m1), ad)))
        out += [_in_range(F, limbs[j], 4) for j in range(31, -1, -1)]
        out.append(F.sub(F.lin([4 ** j for j in range(16)], limbs[:16]), low))
        out.append(F.sub(F.lin([4 ** j for j in range(16)], limbs[16:]), high))
    return out


def _u32_interleave(F, w, k0, k1, pih):
    """U32InterleaveGate, 3 ops: x at 2i, interleaved at 2i + 1, the 32 bits of x at 6 + 32i, most significant first.
    sum 2^k bit_k = x; sum 4^k bit_k = interleaved; the bits are bits."""
    out = []
    for i in range(bw.MULTI_OPS[bw.G_U32_INTERLEAVE]):
        bits = [w[6 + 32 * i + b] for b in range(32)]
        out.append(F.sub(F.lin([1 << (31 - b) for b in range(32)], bits), w[2 * i]))
        out.append(F.sub(F.lin([4 ** (31 - b) for b in range(32)], bits), w[2 * i + 1]))
        out += [_in_range(F, b, 2) for b in bits]
    return out


def _u32_uninterleave(F, w, k0, k1, pih):
    """UninterleaveToU32Gate, 2 ops: x at 3i, evens at 3i + 1, odds at 3i + 2, the 64 bits of x at 6 + 64i, most significant
    first.  The bits give x; those at even positions of that order give `evens` as a 32-bit word, the others `odds`."""
    out = []
    for i in range(bw.MULTI_OPS[bw.G_U32_UNINTERLEAVE]):
        bits = [w[6 + 64 * i + b] for b in range(64)]
        out.append(F.sub(F.lin([1 << (63 - b) for b in range(64)], bits), w[3 * i]))
        weights = [1 << (31 - j) for j in range(32)]
        out.append(F.sub(F.lin(weights, bits[0::2]), w[3 * i + 1]))
        out.append(F.sub(F.lin(weights, bits[1::2]), w[3 * i + 2]))
        out += [_in_range(F, b, 2) for b in bits]
    return out


def _swapped_inputs(F, w, out):
    """The head both permutation gates share: swap (wire 24) is a bit; delta_i (wires 25..28) = swap (in_(i+4) - in_i); the
    state the rounds start from is in_i + delta_i, in_(i+4) - delta_i, in_8 .. in_11."""
    swap = w[24]
    out.append(F.mul(swap, F.sub(swap, F.one)))
    for i in range(4):
        out.append(F.sub(F.mul(swap, F.sub(w[4 + i], w[i])), w[25 + i]))
    return [F.add(w[i], w[25 + i]) for i in range(4)] + [F.sub(w[4 + i], w[25 + i]) for i in range(4)] + [w[i] for i in range(8, 12)]


def _mds(F, s):
    """Poseidon's MDS layer: row r of circ(MDS_CIRC) + diag(8, 0, ..)."""
    return [F.lin(MDS_CIRC + ([MDS_DIAG0] if r == 0 else []), [s[(i + r) % 12] for i in range(12)] + ([s[0]] if r == 0 else []))
            for r in range(12)]


def _poseidon(F, w, k0, k1, pih):
    """PoseidonGate: 30 rounds (4 full, 22 partial, 4 full) of constants, S-box x^7 (all words / word 0), MDS.  Every S-box
    input but those of round 0 is a wire (29.. in round order) the state is checked against and replaced by."""
    out = []
    s = _swapped_inputs(F, w, out)
    wire = 29
    for r in range(30):
        s = [F.add(v, F.k(POSEIDON_RC[12 * r + i])) for i, v in enumerate(s)]
        lanes = range(12) if r < 4 or r >= 26 else range(1)
        for i in lanes:
            if r:
                out.append(F.sub(s[i], w[wire]))
                s[i] = w[wire]
                wire += 1
            s[i] = _pow7(F, s[i])
        s = _mds(F, s)
    assert wire == 135
    return out + [F.sub(s[i], w[12 + i]) for i in range(12)]


def _p2_external(F, s):
    """circ(2 M4, M4, M4): M4 on each block of four, plus the sum of the three blocks' images."""
    y = [F.lin(M4[r], s[4 * b:4 * b + 4]) for b in range(3) for r in range(4)]
    col = [F.add(F.add(y[k], y[4 + k]), y[8 + k]) for k in range(4)]
    return [F.add(y[i], col[i % 4]) for i in range(12)]


def _p2_internal(F, s):
    """1 1^T + diag(mu_i - 1), mu_i - 1 = P2_DIAG_M1[i] - 1."""
    total = F.lin([1] * 12, s)
    return [F.add(F.scale(v, P2_DIAG_M1[i] - 1), total) for i, v in enumerate(s)]


def _poseidon2(F, w, k0, k1, pih):
    """Poseidon2Gate: an external layer, 4 full rounds, 22 partial, 4 full; the S-box inputs of all rounds but the first are
    wires: 29..64 (full rounds 1..3), 65..86 (partial), 87..134 (the last four)."""
    out = []
    s = _p2_external(F, _swapped_inputs(F, w, out))
    for r in range(4):
        s = [F.add(v, F.k(P2_RC[12 * r + i])) for i, v in enumerate(s)]
        if r:
            out += [F.sub(s[i], w[29 + 12 * (r - 1) + i]) for i in range(12)]
            s = [w[29 + 12 * (r - 1) + i] for i in range(12)]
        s = _p2_external(F, [_pow7(F, v) for v in s])
    for r in range(22):
        out.append(F.sub(F.add(s[0], F.k(P2_RC_MID[r])), w[65 + r]))
        s = _p2_internal(F, [_pow7(F, w[65 + r])] + s[1:])
    for r in range(4, 8):
        s = [F.add(v, F.k(P2_RC[12 * r + i])) for i, v in enumerate(s)]
        out += [F.sub(s[i], w[87 + 12 * (r - 4) + i]) for i in range(12)]
        s = _p2_external(F, [_pow7(F, w[87 + 12 * (r - 4) + i]) for i in range(12)])
    return out + [F.sub(s[i], w[12 + i]) for i in range(12)]


def _random_access(F, w, k0, k1, pih):
    """RandomAccessGate (bits 4, 4 copies, 2 extra constants): copy c has index, claimed element and 16 items at 18c, its 4
    index bits (little-endian) at 74 + 4c.  Per copy: the bits are bits; they give the index; the claimed element is the item
    the bits select, as the multilinear sum over the 16 items.  Then the constants at wires 72, 73."""
    out = []
    for c in range(bw.MULTI_OPS[bw.G_RANDOM_ACCESS]):
        bits = [w[74 + bw.RA_BITS * c + b] for b in range(bw.RA_BITS)]
        out += [_in_range(F, b, 2) for b in bits]
        out.append(F.sub(F.lin([1 << b for b in range(bw.RA_BITS)], bits), w[18 * c]))
        chosen = F.zero
        for idx in range(bw.RA_VEC):
            ind = _prod(F, [bits[b] if (idx >> b) & 1 else F.sub(F.one, bits[b]) for b in range(bw.RA_BITS)])
            chosen = F.add(chosen, F.mul(ind, w[18 * c + 2 + idx]))
        out.append(F.sub(chosen, w[18 * c + 1]))
    return out + [F.sub(k0, w[72]), F.sub(k1, w[73])]


def _reducing(F, w, n_coeffs, ext):
    """acc_(i+1) = acc_i alpha + coeff_i in A: output (= the last accumulator) at 0, 1, alpha at 2, 3, acc_0 at 4, 5, the
    coefficients from 6 (single wires, or pairs), then the accumulators but the last."""
    cw = 2 if ext else 1
    alpha, acc = _pair(w, 2), _pair(w, 4)
    out = []
    for i in range(n_coeffs):
        coeff = _pair(w, 6 + 2 * i) if ext else (w[6 + i], F.zero)
        nxt = _pair(w, 0) if i == n_coeffs - 1 else _pair(w, 6 + cw * n_coeffs + 2 * i)
        out += list(_alg_sub(F, _alg_add(F, _alg_mul(F, acc, alpha), coeff), nxt))
        acc = nxt
    return out


def _coset_interp(F, w, k0, k1, pih):
    """CosetInterpolationGate (subgroup_bits 4, degree 6): shift at 0, 16 value pairs at 1, the point at 33, the value at 35,
    the intermediate evaluations at 37 / 39 and products at 41 / 43, the shifted point x = point / shift at 45.
    The barycentric recurrence (eval, prod) -> (eval (x - g^i) + w_i v_i prod, prod (x - g^i)), w_i = g^i / 16, runs over the
    points 0..5, 6..10, 11..15, its state going through wires between the chunks; in closed form a chunk C maps
    (e, p) to (e T + p sum_(i in C) w_i v_i prod_(j in C, j != i) (x - g^j), p T), T = prod_(j in C) (x - g^j)."""
    g, inv16 = bw.root_of_unity(4), pow(16, P - 2, P)
    shift, point, x = w[0], _pair(w, 33), _pair(w, 45)
    out = list(_alg_sub(F, point, _alg_scale(F, x, shift)))
    term = [_alg_sub(F, x, (F.k(pow(g, j, P)), F.zero)) for j in range(16)]
    one = (F.one, F.zero)

    def product(js):
        t = one
        for j in js:
            t = _alg_mul(F, t, term[j])
        return t

    state = ((F.zero, F.zero), one)
    for n, chunk in enumerate((range(0, 6), range(6, 11), range(11, 16))):
        if n:
            wires = (_pair(w, 37 + 2 * (n - 1)), _pair(w, 41 + 2 * (n - 1)))
            out += list(_alg_sub(F, wires[0], state[0])) + list(_alg_sub(F, wires[1], state[1]))
            state = wires
        total = product(chunk)
        s = (F.zero, F.zero)
        for i in chunk:
            v = _alg_scale(F, _pair(w, 1 + 2 * i), F.k(pow(g, i, P) * inv16))
            s = _alg_add(F, s, _alg_mul(F, v, product([j for j in chunk if j != i])))
        state = (_alg_add(F, _alg_mul(F, state[0], total), _alg_mul(F, state[1], s)), _alg_mul(F, state[1], total))
    return out + list(_alg_sub(F, _pair(w, 35), state[0]))


def _poseidon_mds(F, w, k0, k1, pih):
    """PoseidonMdsGate: 12 input pairs at 0, 12 output pairs at 24; the MDS layer acts on each component."""
    comp = [_mds(F, [w[2 * i + d] for i in range(12)]) for d in range(2)]
    return [F.sub(w[24 + 2 * r + d], comp[d][r]) for r in range(12) for d in range(2)]


_MODELS = {
    bw.G_NOOP: _noop, bw.G_CONSTANT: _constant, bw.G_PUBLIC_INPUT: _public_input, bw.G_BASE_SUM: _base_sum,
    bw.G_U32_INTERLEAVE: _u32_interleave, bw.G_U32_UNINTERLEAVE: _u32_uninterleave, bw.G_ARITHMETIC: _arithmetic,
    bw.G_MUL_EXT: _mul_ext, bw.G_EXPONENTIATION: _exponentiation, bw.G_U32_ARITHMETIC: _u32_arithmetic,
    bw.G_POSEIDON2: _poseidon2, bw.G_ARITH_EXT: _arith_ext, bw.G_POSEIDON: _poseidon, bw.G_RANDOM_ACCESS: _random_access,
    bw.G_REDUCING: lambda F, w, k0, k1, pih: _reducing(F, w, bw.RED_COEFFS, False),
    bw.G_REDUCING_EXT: lambda F, w, k0, k1, pih: _reducing(F, w, bw.REDX_COEFFS, True),
    bw.G_COSET_INTERP: _coset_interp, bw.G_POSEIDON_MDS: _poseidon_mds,
}
KINDS = sorted(_MODELS)
assert KINDS == list(range(18)) and set(KINDS) == set(bw.GATE_CONSTRAINTS)


def constraints(kind, F, wires, k0, k1, pi_hash):
    out = _MODELS[kind](F, wires, k0, k1, pi_hash)
    assert len(out) == bw.GATE_CONSTRAINTS[kind], (kind, len(out))
    return out


# (number of leading wire columns read, constants read, reads the public-input hash)
_READS = {
    bw.G_NOOP: (0, (), False), bw.G_CONSTANT: (2, (0, 1), False), bw.G_PUBLIC_INPUT: (4, (), True),
    bw.G_BASE_SUM: (1 + bw.BASE_SUM_LIMBS, (), False), bw.G_U32_INTERLEAVE: (6 + 3 * 32, (), False),
    bw.G_U32_UNINTERLEAVE: (6 + 2 * 64, (), False), bw.G_ARITHMETIC: (4 * bw.ARITH_OPS, (0, 1), False),
    bw.G_MUL_EXT: (6 * 13, (0,), False), bw.G_EXPONENTIATION: (2 + 2 * bw.EXP_BITS, (), False),
    bw.G_U32_ARITHMETIC: (18 + 3 * 32, (), False), bw.G_POSEIDON2: (135, (), False), bw.G_ARITH_EXT: (8 * 10, (0, 1), False),
    bw.G_POSEIDON: (135, (), False), bw.G_RANDOM_ACCESS: (74 + 4 * bw.RA_BITS, (0, 1), False),
    bw.G_REDUCING: (4 + 3 * bw.RED_COEFFS, (), False), bw.G_REDUCING_EXT: (4 + 4 * bw.REDX_COEFFS, (), False),
    bw.G_COSET_INTERP: (47, (), False), bw.G_POSEIDON_MDS: (48, (), False),
}


def reads(kind):
    """{"wires": the wire columns, "consts": the constants (0, 1), "pi": whether the public-input hash} the constraints of
    `kind` depend on.  Every gate reads a prefix of its row."""
    n, consts, pi = _READS[kind]
    return {"wires": list(range(n)), "consts": list(consts), "pi": pi}


def num_wires_read(kinds):
    return max([_READS[k][0] for k in kinds] + [0])
