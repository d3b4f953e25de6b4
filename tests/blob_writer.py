"""An INDEPENDENT writer of the circuit blob (`p25_circuit_import`), in pure Python, following the field-by-field
specification in INTEGRATION.md section 5 -- not the product's `p25_circuit_export`.

It plays the part of the Rust host that keeps `builder.build::<C>()` (/root/reference/src/p3/mod.rs:250) and hands the
resulting `CircuitData` to the library: a miniature circuit builder (arithmetic gates, constants, the public-input
row, copy constraints) that derives selectors, sigma polynomials, k_i's, the representative map and the generator
table by itself and serialises them.  tests/test_blob_independent_writer.py imports its output and proves with it.
"""
import struct

P = 0xFFFFFFFF00000001
MAGIC = b"P25CIRC1"

# gate kinds / generator kinds of the blob (INTEGRATION.md section 5, tables "gate kind" and "generator kind")
G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC = 0, 1, 2, 6
G_U32_INTERLEAVE, G_U32_UNINTERLEAVE, G_U32_ARITHMETIC, G_POSEIDON2 = 4, 5, 9, 10     # the reference's own four gates
G_BASE_SUM, G_MUL_EXT, G_EXPONENTIATION, G_ARITH_EXT, G_POSEIDON = 3, 7, 8, 11, 12
G_RANDOM_ACCESS, G_REDUCING, G_REDUCING_EXT, G_COSET_INTERP, G_POSEIDON_MDS = 13, 14, 15, 16, 17
GEN_CONSTANT, GEN_RANDOM, GEN_ARITHMETIC = 0, 1, 2
GEN_MUL_EXT, GEN_QUOTIENT_EXT, GEN_BASE_SPLIT, GEN_WIRE_SPLIT, GEN_BASE_SUM, GEN_LOW_HIGH, GEN_EXPONENTIATION = 3, 4, 5, 6, 7, 8, 9
GEN_POSEIDON2, GEN_U32_ARITHMETIC, GEN_U32_INTERLEAVE, GEN_U32_UNINTERLEAVE = 10, 11, 12, 13
GEN_ARITH_EXT, GEN_POSEIDON, GEN_RANDOM_ACCESS, GEN_REDUCING, GEN_REDUCING_EXT, GEN_COSET_INTERP, GEN_POSEIDON_MDS = 14, 15, 16, 17, 18, 19, 20
_PHANTOM = "PhantomData<plonky2_field::goldilocks_field::GoldilocksField>"
# (degree, Gate::id()) -- orders the gate set; the reference's ids are `format!("{self:?}")` of its structs
# (interleave_u32.rs:98-100, uninterleave_to_u32.rs:110-112, arithmetic_u32.rs:102-104, poseidon2_gate.rs:146-148)
GATE_ORDER = {
    G_NOOP: (0, "NoopGate"),
    G_CONSTANT: (1, "ConstantGate { num_consts: 2 }"),
    G_PUBLIC_INPUT: (1, "PublicInputGate"),
    G_U32_INTERLEAVE: (2, "U32InterleaveGate { num_ops: 3 }"),
    G_U32_UNINTERLEAVE: (2, "UninterleaveToU32Gate { num_ops: 2 }"),
    G_ARITHMETIC: (3, "ArithmeticGate { num_ops: 20 }"),
    G_U32_ARITHMETIC: (4, "U32ArithmeticGate { num_ops: 3, _phantom: " + _PHANTOM + " }"),
    G_POSEIDON2: (7, "Poseidon2Gate { _phantom: " + _PHANTOM + " }<WIDTH=12>"),
    # upstream's gates: degree() of each gate file, ids as far as INTEGRATION.md section 5 spells them (".." = parameters
    # it leaves out; the names alone already order any two of them, the first differing letter being inside the name)
    G_BASE_SUM: (2, "BaseSumGate { num_limbs: 63 } + Base: 2"),                      # degree = the base B
    G_MUL_EXT: (3, "MulExtensionGate { num_ops: 13 }"),
    G_EXPONENTIATION: (4, "ExponentiationGate { num_power_bits: 66, .. }"),
    G_ARITH_EXT: (3, "ArithmeticExtensionGate { num_ops: 10 }"),
    G_POSEIDON: (7, "PoseidonGate(..)<WIDTH=12>"),
    G_RANDOM_ACCESS: (5, "RandomAccessGate { bits: 4, num_copies: 4, num_extra_constants: 2, .. }<D=2>"),   # bits + 1
    G_REDUCING: (2, "ReducingGate { num_coeffs: 43 }"),
    G_REDUCING_EXT: (2, "ReducingExtensionGate { num_coeffs: 32 }"),
    G_COSET_INTERP: (6, "CosetInterpolationGate { subgroup_bits: 4, degree: 6, .. }<D=2>"),                # its `degree`
    G_POSEIDON_MDS: (1, "PoseidonMdsGate(..)<WIDTH=12>"),
}
# num_constraints of the reference's gates: interleave_u32.rs:229-231 (num_ops * (2 + 32)), uninterleave_to_u32.rs:264-266
# (num_ops * (3 + 64)), arithmetic_u32.rs:167-169 (num_ops * (4 + 32)), poseidon2_gate.rs:425-427 (1 + 4 + 12 * 3 + 22 + 12 * 4 + 12)
GATE_CONSTRAINTS = {G_NOOP: 0, G_CONSTANT: 2, G_PUBLIC_INPUT: 4, G_ARITHMETIC: 20, G_U32_INTERLEAVE: 3 * 34,
                    G_U32_UNINTERLEAVE: 2 * 67, G_U32_ARITHMETIC: 3 * 36, G_POSEIDON2: 123,
                    # upstream: one sum + 63 limb checks; 2 per extension op; 66 steps + the output; Poseidon as its clone
                    # Poseidon2; per copy 4 bit checks + index + claimed element, + 2 extra constants; 2 per accumulator;
                    # the shifted point + two intermediate (evaluation, product) states + the value, 2 words each; 12 x 2
                    G_BASE_SUM: 1 + 63, G_MUL_EXT: 13 * 2, G_EXPONENTIATION: 66 + 1, G_ARITH_EXT: 10 * 2, G_POSEIDON: 123,
                    G_RANDOM_ACCESS: 4 * (4 + 2) + 2, G_REDUCING: 43 * 2, G_REDUCING_EXT: 32 * 2,
                    G_COSET_INTERP: 2 + 2 * 4 + 2, G_POSEIDON_MDS: 24}
# ops per row (num_ops at 135 wires / 80 routed)
MULTI_OPS = {G_U32_INTERLEAVE: 3, G_U32_UNINTERLEAVE: 2, G_U32_ARITHMETIC: 3, G_RANDOM_ACCESS: 4}
EXT_OPS = {G_MUL_EXT: (13, 6), G_ARITH_EXT: (10, 8)}      # (ops per row, wires per op) of the gates with per-row constants
BASE_SUM_LIMBS, EXP_BITS, RA_BITS, RA_VEC, RED_COEFFS, REDX_COEFFS = 63, 66, 4, 16, 43, 32
MAX_DEGREE = 9                                       # max_quotient_degree_factor + 1 (upstream selectors.rs)
UNUSED_SELECTOR = 0xFFFFFFFF
NUM_WIRES, NUM_ROUTED, NUM_CONSTANTS, ARITH_OPS = 135, 80, 2, 20   # CircuitConfig::standard_recursion_config()


def root_of_unity(log_n):
    g = 1753635133440165772                    # 7^((p-1)/2^32): two_adic.rs:35
    for _ in range(32 - log_n):
        g = g * g % P
    return g


class MiniCircuit:
    """Targets are ("v", i) virtual or ("w", row, col) wires.

    num_wires, num_routed, rate_bits, num_constants: the CircuitConfig fields a blob's header carries (defaults:
    standard_recursion_config); constant polynomials beyond the two the gates use are zero.
    The gates keep the parameters their blob kinds name (ArithmeticGate { num_ops: 20 } and so on) under every
    configuration: the library refuses a gate that needs more wires than num_wires, and a copy constraint on a column
    that is not routed is refused here."""

    def __init__(self, num_wires=NUM_WIRES, num_routed=NUM_ROUTED, rate_bits=3, num_constants=NUM_CONSTANTS):
        assert 1 <= num_routed <= num_wires and rate_bits >= 3 and num_constants >= NUM_CONSTANTS
        self.num_wires, self.num_routed, self.rate_bits, self.num_constants = num_wires, num_routed, rate_bits, num_constants
        self.rows = []                 # [kind, c0, c1]
        self.copies = []
        self.n_virtual = 0
        self.inputs = []
        self.constants = {}            # value -> target
        self.open_arith = {}           # (c0, c1) -> (row, next op)
        self.open_ops = {}             # multi-op gate kind -> (row, next op)   (CircuitBuilder::find_slot)
        self.generators = []           # (kind, c0, c1, aux, deps, outs)
        self.open_ext = {}             # (extension gate kind, c0, c1) -> (row, next op)
        self.base_sum_limbs = {}       # BaseSum row -> limbs its BaseSplitGenerator writes

    def virtual(self):
        self.n_virtual += 1
        return ("v", self.n_virtual - 1)

    def input(self):
        t = self.virtual()
        self.inputs.append(t)
        return t

    def constant(self, v):
        if v not in self.constants:
            self.constants[v] = self.virtual()
        return self.constants[v]

    def connect(self, a, b):
        self.copies.append((a, b))

    def arithmetic(self, c0, c1, m0, m1, addend):
        """ArithmeticGate op: out = c0*m0*m1 + c1*addend (one open row per (c0, c1), as CircuitBuilder::find_slot)."""
        self.constant(0)                                   # upstream's special-case analysis touches zero()
        key = (c0, c1)
        if key in self.open_arith:
            row, op = self.open_arith[key]
        else:
            row, op = len(self.rows), 0
            self.rows.append([G_ARITHMETIC, c0, c1])
        if op == ARITH_OPS - 1:
            self.open_arith.pop(key, None)
        else:
            self.open_arith[key] = (row, op + 1)
        for k, t in enumerate((m0, m1, addend)):
            self.connect(t, ("w", row, 4 * op + k))
        return ("w", row, 4 * op + 3)

    def mul(self, a, b):
        return self.arithmetic(1, 0, a, b, a)

    def add(self, a, b):
        return self.arithmetic(1, 1, a, self.constant(1), b)

    # ---- the reference's gates (wire layouts from their `wire_*` accessors)
    def _slot(self, kind):
        if kind in self.open_ops:
            row, op = self.open_ops[kind]
        else:
            row, op = len(self.rows), 0
            self.rows.append([kind, 0, 0])
        if op == MULTI_OPS[kind] - 1:
            self.open_ops.pop(kind, None)
        else:
            self.open_ops[kind] = (row, op + 1)
        return row, op

    def interleave_u32(self, x):
        """gadgets/interleaved_u32.rs:89-111 on a U32InterleaveGate op: wires 2i (x) and 2i + 1 (interleaved) (interleave_u32.rs:45-62)."""
        row, i = self._slot(G_U32_INTERLEAVE)
        self.connect(("w", row, 2 * i), x)
        return ("w", row, 2 * i + 1)

    def uninterleave_to_u32(self, x):
        """UninterleaveToU32Gate op: wires 3i (x), 3i + 1 (evens), 3i + 2 (odds) (uninterleave_to_u32.rs:47-75)."""
        row, i = self._slot(G_U32_UNINTERLEAVE)
        self.connect(("w", row, 3 * i), x)
        return ("w", row, 3 * i + 1), ("w", row, 3 * i + 2)

    def mul_add_u32(self, x, y, z):
        """U32ArithmeticGate op: wires 6i, 6i + 1, 6i + 2 (multiplicands, addend), 6i + 3 / 6i + 4 (low, high) (arithmetic_u32.rs:40-80)."""
        row, i = self._slot(G_U32_ARITHMETIC)
        for k, t in enumerate((x, y, z)):
            self.connect(("w", row, 6 * i + k), t)
        return ("w", row, 6 * i + 3), ("w", row, 6 * i + 4)

    def poseidon2_permute(self, state):
        """Poseidon2Hash::permute_targets (poseidon2.rs:585-609): one Poseidon2Gate row, swap = 0, inputs 0..11, outputs 12..23."""
        row = len(self.rows)
        self.rows.append([G_POSEIDON2, 0, 0])
        self.connect(self.constant(0), ("w", row, 24))
        for i, t in enumerate(state):
            self.connect(t, ("w", row, i))
        return [("w", row, 12 + i) for i in range(12)]

    # ---- upstream's remaining gates (wire layouts: INTEGRATION.md section 5a.1, "deps -> outs as wire columns of row")
    def _ext_slot(self, kind, c0, c1):
        ops, _w = EXT_OPS[kind]
        key = (kind, c0, c1)
        if key in self.open_ext:
            row, op = self.open_ext[key]
        else:
            row, op = len(self.rows), 0
            self.rows.append([kind, c0, c1])
        if op == ops - 1:
            self.open_ext.pop(key, None)
        else:
            self.open_ext[key] = (row, op + 1)
        return row, op

    def mul_extension(self, c0, a, b):
        """MulExtensionGate op: out = c0 * a * b in F_p^2; a, b pairs of targets; wires 6i..6i+3 -> 6i+4, 6i+5."""
        row, i = self._ext_slot(G_MUL_EXT, c0, 0)
        for k, t in enumerate(tuple(a) + tuple(b)):
            self.connect(t, ("w", row, 6 * i + k))
        return ("w", row, 6 * i + 4), ("w", row, 6 * i + 5)

    def arithmetic_extension(self, c0, c1, m0, m1, addend):
        """ArithmeticExtensionGate op: out = c0 * m0 * m1 + c1 * addend in F_p^2; wires 8i..8i+5 -> 8i+6, 8i+7."""
        row, i = self._ext_slot(G_ARITH_EXT, c0, c1)
        for k, t in enumerate(tuple(m0) + tuple(m1) + tuple(addend)):
            self.connect(t, ("w", row, 8 * i + k))
        return ("w", row, 8 * i + 6), ("w", row, 8 * i + 7)

    def div_extension(self, num, den):
        """upstream div_extension: QuotientGeneratorExtension writes q = num / den into two virtual targets, and the circuit
        holds q * den == num (here with a MulExtensionGate op)."""
        q = (self.virtual(), self.virtual())
        self.generators.append((GEN_QUOTIENT_EXT, 0, 0, 0, list(num) + list(den), list(q)))
        back = self.mul_extension(1, q, den)
        for t, u in zip(back, num):
            self.connect(t, u)
        return q

    def base_sum_row(self, n_limbs):
        """A BaseSumGate<2> row (63 limbs) used for n_limbs of them: wire 0 the sum, wires 1.. the little-endian bits; the
        row's BaseSplitGenerator writes n_limbs bits and the limbs above are connected to zero.  -> (sum, bits)"""
        assert 1 <= n_limbs <= BASE_SUM_LIMBS
        row = len(self.rows)
        self.rows.append([G_BASE_SUM, 0, 0])
        self.base_sum_limbs[row] = n_limbs
        zero = self.constant(0)
        for k in range(n_limbs, BASE_SUM_LIMBS):
            self.connect(zero, ("w", row, 1 + k))
        return ("w", row, 0), [("w", row, 1 + k) for k in range(n_limbs)]

    def range_check(self, x, n_bits):
        s, bits = self.base_sum_row(n_bits)
        self.connect(x, s)
        return bits

    def le_sum(self, bits):
        """upstream le_sum: the bits connected to the limbs of a BaseSum row, BaseSumGenerator bits -> sum."""
        s, limbs = self.base_sum_row(len(bits))
        for b, l in zip(bits, limbs):
            self.connect(b, l)
        self.generators.append((GEN_BASE_SUM, 0, 0, 0, list(bits), [s]))
        return s

    def split_le_64(self, x):
        """upstream split_le(x, 64): two BaseSum rows (63 bits + 1 bit), WireSplitGenerator x -> the two 63-bit chunks,
        chunk_1 * 2^63 + chunk_0 connected to x.  -> the 64 bits, little-endian"""
        s0, b0 = self.base_sum_row(BASE_SUM_LIMBS)
        s1, b1 = self.base_sum_row(1)
        self.generators.append((GEN_WIRE_SPLIT, 0, 0, 0, [x], [s0, s1]))
        self.connect(self.arithmetic(1 << 63, 1, s1, self.constant(1), s0), x)
        return b0 + b1

    def split_low_high(self, x, n_log, num_bits=64):
        """upstream split_low_high: LowHighGenerator x -> low (n_log bits), high; both range-checked on BaseSum rows and
        high * 2^n_log + low connected to x.  -> (low, high)"""
        low, high = self.virtual(), self.virtual()
        self.generators.append((GEN_LOW_HIGH, 0, 0, n_log, [x], [low, high]))
        self.range_check(low, n_log)
        self.range_check(high, num_bits - n_log)
        self.connect(self.arithmetic(1, 1, high, self.constant(1 << n_log), low), x)
        return low, high

    def exponentiation(self, base, bits):
        """ExponentiationGate row: wire 0 the base, 1..66 the exponent's bits (little-endian), 67 the output, 68..133 the
        intermediate values (most significant bit first)."""
        assert len(bits) == EXP_BITS
        row = len(self.rows)
        self.rows.append([G_EXPONENTIATION, 0, 0])
        self.connect(base, ("w", row, 0))
        for k, b in enumerate(bits):
            self.connect(b, ("w", row, 1 + k))
        return ("w", row, 67), [("w", row, 68 + k) for k in range(EXP_BITS)]

    def _permutation_row(self, kind, state, swap):
        row = len(self.rows)
        self.rows.append([kind, 0, 0])
        self.connect(swap, ("w", row, 24))
        for i, t in enumerate(state):
            self.connect(t, ("w", row, i))
        return row

    def poseidon2_row(self, state, swap):
        """A Poseidon2Gate row with a swap target of the caller's.  -> the row"""
        return self._permutation_row(G_POSEIDON2, state, swap)

    def poseidon_row(self, state, swap):
        """A PoseidonGate row: the wire layout its clone Poseidon2Gate has (inputs 0..11, outputs 12..23, swap 24, deltas
        25..28, S-box inputs 29..134).  -> the row"""
        return self._permutation_row(G_POSEIDON, state, swap)

    def random_access(self, index, items, extra_constants=(0, 0)):
        """RandomAccessGate copy c: wire 18c the index, 18c+1 the claimed element, 18c+2..18c+17 the list, 74+4c.. the
        index bits; wires 72, 73 hold the row's two constants.  -> the claimed element"""
        assert len(items) == RA_VEC
        fresh = G_RANDOM_ACCESS not in self.open_ops
        row, c = self._slot(G_RANDOM_ACCESS)
        if fresh:
            self.rows[row][1:] = list(extra_constants)
        self.connect(index, ("w", row, 18 * c))
        for k, t in enumerate(items):
            self.connect(t, ("w", row, 18 * c + 2 + k))
        return ("w", row, 18 * c + 1)

    def reducing(self, alpha, old_acc, coeffs, ext=False):
        """ReducingGate (43 base coefficients) / ReducingExtensionGate (32 pairs): wires 0, 1 the output, 2, 3 alpha, 4, 5
        the old accumulator, 6.. the coefficients, then the accumulators but the last.  -> (output pair, accumulator wires)"""
        n, w = (REDX_COEFFS, 2) if ext else (RED_COEFFS, 1)
        flat = [t for c in coeffs for t in c] if ext else list(coeffs)
        assert len(flat) == n * w
        row = len(self.rows)
        self.rows.append([G_REDUCING_EXT if ext else G_REDUCING, 0, 0])
        for k, t in enumerate(list(alpha) + list(old_acc) + flat):
            self.connect(t, ("w", row, 2 + k))
        accs = [("w", row, 6 + n * w + k) for k in range(2 * (n - 1))] + [("w", row, 0), ("w", row, 1)]
        return (("w", row, 0), ("w", row, 1)), accs

    def coset_interpolation(self, shift, values, point):
        """CosetInterpolationGate(subgroup_bits 4, degree 6): wire 0 the shift, 1..32 the 16 value pairs, 33, 34 the point,
        35, 36 the value, 37..44 the intermediate states, 45, 46 the shifted point.  -> (value pair, the generator's outputs)"""
        row = len(self.rows)
        self.rows.append([G_COSET_INTERP, 0, 0])
        flat = [shift] + [t for v in values for t in v] + list(point)
        assert len(flat) == 35
        for k, t in enumerate(flat):
            self.connect(t, ("w", row, k))
        return (("w", row, 35), ("w", row, 36)), [("w", row, k) for k in (45, 46, 37, 38, 41, 42, 39, 40, 43, 44, 35, 36)]

    def poseidon_mds(self, state):
        """PoseidonMdsGate: 12 input pairs on wires 0..23 -> 12 output pairs on wires 24..47."""
        row = len(self.rows)
        self.rows.append([G_POSEIDON_MDS, 0, 0])
        for k, t in enumerate([t for s in state for t in s]):
            self.connect(t, ("w", row, k))
        return [("w", row, 24 + k) for k in range(24)]

    # ------------------------------------------------------------------ build(): the tables of the blob
    def build(self):
        rows = [list(r) for r in self.rows]
        copies = list(self.copies)
        gens = list(self.generators)
        # PublicInputGate: hash of the (empty) public inputs = 4 zeros; unused wires get RandomValueGenerators
        zero = self.constant(0)
        pi_row = len(rows)
        rows.append([G_PUBLIC_INPUT, 0, 0])
        for i in range(4):
            copies.append((zero, ("w", pi_row, i)))
        for w in range(4, self.num_wires):
            gens.append((GEN_RANDOM, 0, 0, w, [], [("w", pi_row, w)]))
        # ConstantGates: constants in increasing order, two per row
        consts = sorted(self.constants.items())
        for k, (val, t) in enumerate(consts):
            if k % NUM_CONSTANTS == 0:
                rows.append([G_CONSTANT, 0, 0])
            row = len(rows) - 1
            rows[row][1 + k % NUM_CONSTANTS] = val
            copies.append((("w", row, k % NUM_CONSTANTS), t))
            gens.append((GEN_CONSTANT, val, 0, 0, [], [("w", row, k % NUM_CONSTANTS)]))
        while len(rows) & (len(rows) - 1):
            rows.append([G_NOOP, 0, 0])
        n = len(rows)
        degree_bits = n.bit_length() - 1
        W, RW = self.num_wires, self.num_routed
        for a, b in copies:                                 # the permutation argument covers the routed columns alone
            assert all(t[0] == "v" or t[2] < RW for t in (a, b)), (a, b)

        def tidx(t):
            return n * W + t[1] if t[0] == "v" else t[1] * W + t[2]

        n_targets = n * W + self.n_virtual
        # gate set sorted by (degree, id); one selector group when max_degree + num_gates - 1 <= 9
        kinds = sorted({r[0] for r in rows}, key=lambda k: GATE_ORDER[k])
        gate_index = {k: i for i, k in enumerate(kinds)}
        # selector polynomials (upstream selectors.rs::selector_polynomials): one if everything fits the degree bound, else
        # greedy groups -- gates are taken while (gates in the group) + (degree of the next gate) < max_degree
        degs = [GATE_ORDER[k][0] for k in kinds]
        if degs[-1] + len(kinds) - 1 <= MAX_DEGREE:
            groups = [(0, len(kinds))]
        else:
            groups, start = [], 0
            while start < len(kinds):
                size = 0
                while start + size < len(kinds) and size + degs[start + size] < MAX_DEGREE:
                    size += 1
                assert size > 0
                groups.append((start, start + size))
                start += size
        group_of = [next(g for g, (a, b) in enumerate(groups) if a <= i < b) for i in range(len(kinds))]
        if len(groups) == 1:
            selectors = [[gate_index[r[0]] for r in rows]]
        else:
            selectors = [[gate_index[r[0]] if group_of[gate_index[r[0]]] == g else UNUSED_SELECTOR for r in rows]
                         for g in range(len(groups))]
        const_polys = [[r[1] for r in rows], [r[2] for r in rows]] + [[0] * n for _ in range(self.num_constants - NUM_CONSTANTS)]
        # copy constraints -> partitions -> sigma polynomials
        parent = list(range(n_targets))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b in copies:
            ra, rb = find(tidx(a)), find(tidx(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)           # any representative is valid; this one differs from the product's
        rep = [find(i) for i in range(n_targets)]
        k_is = [pow(7, i, P) for i in range(RW)]
        w_n = root_of_unity(degree_bits)
        subgroup = [pow(w_n, i, P) for i in range(n)]
        members = {}
        for row in range(n):
            for col in range(RW):
                members.setdefault(rep[row * W + col], []).append((row, col))
        nxt = {}
        for cyc in members.values():                        # next wire of the partition in (row, col) order, cyclic
            for i, rc in enumerate(cyc):
                nxt[rc] = cyc[(i + 1) % len(cyc)]
        sigmas = [[k_is[nxt[(row, col)][1]] * subgroup[nxt[(row, col)][0]] % P for row in range(n)]
                  for col in range(RW)]
        # per-row gate generators after the explicit ones; unused ops of an incomplete row are dropped
        used_ops = {row: op for (row, op) in self.open_arith.values()}
        used_ops.update({row: op for (row, op) in self.open_ops.values()})
        used_ops.update({row: op for (row, op) in self.open_ext.values()})

        def w(row, col):
            return ("w", row, col)

        for row, r in enumerate(rows):
            if r[0] == G_ARITHMETIC:
                for i in range(used_ops.get(row, ARITH_OPS)):
                    gens.append((GEN_ARITHMETIC, r[1], r[2], 0, [("w", row, 4 * i + k) for k in range(3)],
                                 [("w", row, 4 * i + 3)]))
            elif r[0] == G_U32_INTERLEAVE:      # interleave_u32.rs:305-334: x -> 32 bits (wires 6 + 32 i ..), interleaved
                for i in range(used_ops.get(row, 3)):
                    gens.append((GEN_U32_INTERLEAVE, 0, 0, 0, [w(row, 2 * i)],
                                 [w(row, 6 + 32 * i + j) for j in range(32)] + [w(row, 2 * i + 1)]))
            elif r[0] == G_U32_UNINTERLEAVE:    # uninterleave_to_u32.rs:353-390: x -> 64 bits (wires 6 + 64 i ..), evens, odds
                for i in range(used_ops.get(row, 2)):
                    gens.append((GEN_U32_UNINTERLEAVE, 0, 0, 0, [w(row, 3 * i)],
                                 [w(row, 6 + 64 * i + j) for j in range(64)] + [w(row, 3 * i + 1), w(row, 3 * i + 2)]))
            elif r[0] == G_U32_ARITHMETIC:      # arithmetic_u32.rs:389-439: m0, m1, addend -> low, high, inverse, 32 limbs (wires 18 + 32 i ..)
                for i in range(used_ops.get(row, 3)):
                    gens.append((GEN_U32_ARITHMETIC, 0, 0, 0, [w(row, 6 * i + k) for k in range(3)],
                                 [w(row, 6 * i + 3), w(row, 6 * i + 4), w(row, 6 * i + 5)] + [w(row, 18 + 32 * i + j) for j in range(32)]))
            elif r[0] == G_POSEIDON2:           # poseidon2_gate.rs:447-523: 12 inputs, swap -> 4 deltas, 106 S-box inputs, 12 outputs
                gens.append((GEN_POSEIDON2, 0, 0, 0, [w(row, k) for k in range(12)] + [w(row, 24)],
                             [w(row, 25 + k) for k in range(4)] + [w(row, 29 + k) for k in range(106)] + [w(row, 12 + k) for k in range(12)]))
            elif r[0] == G_POSEIDON:            # PoseidonGenerator: the same record under kind 15
                gens.append((GEN_POSEIDON, 0, 0, 0, [w(row, k) for k in range(12)] + [w(row, 24)],
                             [w(row, 25 + k) for k in range(4)] + [w(row, 29 + k) for k in range(106)] + [w(row, 12 + k) for k in range(12)]))
            elif r[0] == G_BASE_SUM:            # BaseSplitGenerator<2>: sum -> limbs
                gens.append((GEN_BASE_SPLIT, 0, 0, 0, [w(row, 0)], [w(row, 1 + k) for k in range(self.base_sum_limbs[row])]))
            elif r[0] == G_MUL_EXT:             # MulExtensionGenerator: c0; 6i..6i+3 -> 6i+4, 6i+5
                for i in range(used_ops.get(row, 13)):
                    gens.append((GEN_MUL_EXT, r[1], 0, 0, [w(row, 6 * i + k) for k in range(4)], [w(row, 6 * i + 4), w(row, 6 * i + 5)]))
            elif r[0] == G_ARITH_EXT:           # ArithmeticExtensionGenerator: c0, c1; 8i..8i+5 -> 8i+6, 8i+7
                for i in range(used_ops.get(row, 10)):
                    gens.append((GEN_ARITH_EXT, r[1], r[2], 0, [w(row, 8 * i + k) for k in range(6)], [w(row, 8 * i + 6), w(row, 8 * i + 7)]))
            elif r[0] == G_EXPONENTIATION:      # ExponentiationGenerator: 0..66 -> 68..133, then 67
                gens.append((GEN_EXPONENTIATION, 0, 0, 0, [w(row, k) for k in range(1 + EXP_BITS)],
                             [w(row, 68 + k) for k in range(EXP_BITS)] + [w(row, 67)]))
            elif r[0] == G_RANDOM_ACCESS:       # per copy 18c, 18c+2..18c+17 -> 18c+1, 74+4c..; the extra constants' generators
                for c in range(used_ops.get(row, 4)):
                    gens.append((GEN_RANDOM_ACCESS, 0, 0, 0, [w(row, 18 * c)] + [w(row, 18 * c + 2 + k) for k in range(RA_VEC)],
                                 [w(row, 18 * c + 1)] + [w(row, 74 + RA_BITS * c + k) for k in range(RA_BITS)]))
                for k in range(2):
                    gens.append((GEN_CONSTANT, r[1 + k], 0, 0, [], [w(row, 72 + k)]))
            elif r[0] in (G_REDUCING, G_REDUCING_EXT):   # 2..5+N w -> accumulator pairs at 6+N w+2k, the last one at 0, 1
                n_co, cw = (REDX_COEFFS, 2) if r[0] == G_REDUCING_EXT else (RED_COEFFS, 1)
                gens.append((GEN_REDUCING_EXT if cw == 2 else GEN_REDUCING, 0, 0, 0, [w(row, 2 + k) for k in range(4 + n_co * cw)],
                             [w(row, 6 + n_co * cw + k) for k in range(2 * (n_co - 1))] + [w(row, 0), w(row, 1)]))
            elif r[0] == G_COSET_INTERP:        # InterpolationGenerator: 0..34 -> 45, 46, 37, 38, 41, 42, 39, 40, 43, 44, 35, 36
                gens.append((GEN_COSET_INTERP, 0, 0, 0, [w(row, k) for k in range(35)],
                             [w(row, k) for k in (45, 46, 37, 38, 41, 42, 39, 40, 43, 44, 35, 36)]))
            elif r[0] == G_POSEIDON_MDS:        # PoseidonMdsGenerator: 0..23 -> 24..47
                gens.append((GEN_POSEIDON_MDS, 0, 0, 0, [w(row, k) for k in range(24)], [w(row, 24 + k) for k in range(24)]))
        # FRI schedule: ConstantArityBits(4, 5) under cap_height 4
        arity, db = [], degree_bits
        while db > 5 and db + self.rate_bits - 4 >= 4:
            arity.append(4)
            db -= 4
        return dict(degree_bits=degree_bits, rows=rows, kinds=kinds, selectors=selectors, groups=groups, group_of=group_of, const_polys=const_polys,
                    sigmas=sigmas, k_is=k_is, rep=rep, gens=gens, pi_row=pi_row, arity=arity,
                    inputs=[tidx(t) for t in self.inputs], tidx=tidx, n_virtual=self.n_virtual,
                    num_wires=W, num_routed=RW, rate_bits=self.rate_bits)

    # ------------------------------------------------------------------ serialisation
    def to_blob(self):
        b = self.build()
        n = 1 << b["degree_bits"]
        out = bytearray(MAGIC)

        def u64s(vals):
            out.extend(struct.pack(f"<{len(vals)}Q", *vals))

        def u32s(vals):
            out.extend(struct.pack(f"<{len(vals)}I", *vals))
            if len(vals) % 2:
                out.extend(b"\0\0\0\0")                     # u32 arrays are padded to 8 bytes

        kinds = b["kinds"]
        header = [0] * 32
        header[0] = b["degree_bits"]
        header[1], header[2], header[3] = self.num_wires, self.num_routed, self.num_constants
        header[4], header[5], header[6], header[7] = 2, 8, self.rate_bits, 4   # challenges, max quotient degree factor (2^min(rate_bits, 3)), rate_bits, cap_height
        header[8], header[9] = 16, 28                                # proof_of_work_bits, num_query_rounds
        header[10] = len(b["arity"])
        header[11] = len(b["selectors"])                             # selector polynomials
        header[12] = max(GATE_CONSTRAINTS[k] for k in kinds)
        header[13] = -(-self.num_routed // 8) - 1                        # partial products per challenge
        header[14] = len(kinds)
        header[15] = b["pi_row"]
        header[16] = b["n_virtual"]
        header[17] = len(b["inputs"])
        header[18] = len(b["gens"])
        header[19] = len(b["selectors"]) + self.num_constants + self.num_routed
        header[20], header[21] = 4, 5                                # FRI ConstantArityBits(4, 5)
        u64s(header)
        for i, k in enumerate(kinds):
            g = b["group_of"][i]
            u64s([k, g, b["groups"][g][0], b["groups"][g][1]])         # kind, selector index, group [start, end)
        u64s(b["arity"])
        u32s([r[0] for r in b["rows"]])
        for p in b["selectors"]:
            u64s(p)
        for p in b["const_polys"]:
            u64s(p)
        for p in b["sigmas"]:
            u64s(p)
        u64s(b["k_is"])
        u32s(b["inputs"])
        u32s(b["rep"])
        for kind, c0, c1, aux, deps, outs in b["gens"]:
            u64s([kind, c0, c1, aux, len(deps), len(outs)])
            u32s([b["tidx"](t) for t in deps] + [b["tidx"](t) for t in outs])
        assert n == len(b["rows"])
        return bytes(out)


def connected_inputs_product():
    """The circuit of p25_circuit_build_gadget(8): inputs a, b, expected; connect(a, b); a*b == expected."""
    c = MiniCircuit()
    a, b, expected = c.input(), c.input(), c.input()
    c.connect(a, b)
    c.connect(c.mul(a, b), expected)
    return c


def sum_of_products(k):
    """A circuit the library has no builder for: inputs x_0..x_{2k-1}, y; sum_i x_{2i}*x_{2i+1} == y (k products and
    k-1 additions: two ArithmeticGate rows with different constants, 2k+1 inputs)."""
    c = MiniCircuit()
    xs = [c.input() for _ in range(2 * k)]
    y = c.input()
    acc = c.mul(xs[0], xs[1])
    for i in range(1, k):
        acc = c.add(acc, c.mul(xs[2 * i], xs[2 * i + 1]))
    c.connect(acc, y)
    return c


def reference_gates():
    """The circuit of p25_circuit_build_gadget(14): the reference's four gates + ArithmeticGate (8 gate types, two selector groups)."""
    c = MiniCircuit()
    x, y, z = c.input(), c.input(), c.input()
    m = c.mul(x, y)
    xi = c.interleave_u32(x)
    yi = c.interleave_u32(y)
    ev, od = c.uninterleave_to_u32(xi)
    lo, hi = c.mul_add_u32(x, y, z)
    zero = c.constant(0)
    out = c.poseidon2_permute([m, xi, yi, ev, od, lo, hi, x, zero, zero, zero, zero])
    for t in (m, xi, yi, ev, od, lo, hi):
        c.connect(t, c.input())
    for i in range(4):
        c.connect(out[i], c.input())
    return c
