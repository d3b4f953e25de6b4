"""GPU: every stage kernel on boundary-valued Goldilocks operands (tests/edge_values.py), through the C ABI.

The other GPU tests feed the kernels uniform field elements or a satisfied witness; the rare paths of the lazy
arithmetic (a correction that fires, a carry across the 32-bit halves, a sum landing exactly on p, a dropped canon)
then have probability about 2^-32 per operation.  Here every input word is 0, 1, p - 1, 2^32 +- 1, ... or within 2^32 of
p, and the structured fills keep the intermediate values of a transform on equal operands and exact zeros.

All comparisons are exact and every output word is also asserted canonical (< p).  References: Python integers at the
sizes they can afford, closed forms at full size, and the oracle elsewhere -- whose answers on this kind of data
tests/test_edge_values_cpu.py checks against the Python forms.
"""
import numpy as np
import pytest

import edge_values as ev
import stage_circuits
from edge_values import EDGE, EPS, P

pytestmark = pytest.mark.gpu
PU = np.uint64(P)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got < PU).all(), (what, "non-canonical output word at", np.argwhere(got >= PU)[:5].tolist())
    diff = np.argwhere(got != want)
    assert diff.size == 0, (what, "first differing words", diff[:5].tolist(), len(diff), "of", got.size)


def _one_hot_states(v):
    s = np.zeros((12, 12), dtype=np.uint64)
    s[np.arange(12), np.arange(12)] = v
    return s


def _hash_states():
    parts = [gen(12 * 3000, 60 + k).reshape(-1, 12) for k, gen in enumerate(ev.GENERATORS.values())]
    parts += [ev.const(12, P - 1).reshape(1, 12), ev.const(12, 0).reshape(1, 12), _one_hot_states(P - 1), _one_hot_states(1),
              ev.alternating(12, P - 1, 0).reshape(1, 12), ev.alternating(12, EPS, P - EPS).reshape(1, 12)]
    parts += [ev.const(12, v).reshape(1, 12) for v in EDGE]
    return np.concatenate(parts)


# ---- hash kernels -------------------------------------------------------------------------------------------------------
def test_poseidon_permute_on_edge_states(gpu, oracle):
    s = _hash_states()
    _same(gpu.poseidon_permute(s), oracle.poseidon_permute(s), "poseidon_permute")


def test_poseidon2_permute_on_edge_states(gpu, oracle):
    s = _hash_states()
    _same(gpu.poseidon2_permute(s), oracle.poseidon2_permute(s), "poseidon2_permute")


# kernels_hash.hip: a level with at most COOP_PARENTS_BATCH parents runs on k_tree_level_coop, a larger one on
# k_tree_level, and once a cap entry has at most TOP_MAX_NODES nodes under it k_tree_top_coop finishes the tree.
COOP_PARENTS_BATCH, TOP_MAX_NODES = 512, 32
MERKLE_SHAPES = [
    (TOP_MAX_NODES << 2, 2),              # 128 leaves, 4 cap entries of exactly TOP_MAX_NODES nodes: the fused top alone
    (2 * COOP_PARENTS_BATCH, 0),          # 1024 leaves: the first level has exactly COOP_PARENTS_BATCH parents (cooperative)
    (4 * COOP_PARENTS_BATCH, 4),          # 2048 leaves: one per-lane level (1024 parents), one cooperative, then the top
    (8 * COOP_PARENTS_BATCH, 0),          # 4096 leaves: two per-lane levels, four cooperative ones, the top
]
# launch_merkle_tree: k_hash_leaves below width 128, k_hash_leaves_wide from 128; 7 / 8 / 9 straddle the sponge rate
MERKLE_WIDTHS = [1, 7, 8, 9, 127, 128, 135]


@pytest.mark.parametrize("n_leaves,cap_height", MERKLE_SHAPES)
@pytest.mark.parametrize("width", MERKLE_WIDTHS)
def test_merkle_commit_on_edge_leaves(gpu, oracle, width, n_leaves, cap_height):
    for name, leaves in (("edge", ev.edge(n_leaves * width, 7 * width + cap_height).reshape(n_leaves, width)),
                         ("mixed", ev.mixed(n_leaves * width, 9 * width + cap_height).reshape(n_leaves, width)),
                         ("const(p-1)", ev.const(n_leaves * width, P - 1).reshape(n_leaves, width))):
        cap_o, tree_o = oracle.merkle_commit(leaves, cap_height, want_tree=True)
        cap_g, tree_g = gpu.merkle_commit(np.ascontiguousarray(leaves.T), cap_height, want_tree=True)
        _same(tree_g, tree_o, ("merkle tree", name, width, n_leaves))
        _same(cap_g, cap_o, ("merkle cap", name, width, n_leaves))


def test_transcript_on_edge_observations(gpu, oracle):
    """The segment lengths of test_transcript_scripts_vs_oracle, every observed word a boundary word."""
    n_obs = [0, 1, 3, 7, 8, 9, 15, 16, 17, 64, 100, 327]
    n_ch = [0, 1, 2, 4, 7, 8, 9, 29]
    for k, (gname, gen) in enumerate(list(ev.GENERATORS.items()) + [("const(p-1)", lambda n, _s: ev.const(n, P - 1)),
                                                                    ("const(0)", lambda n, _s: ev.const(n, 0))]):
        for trial in range(4):
            segs = [(gen(n_obs[(5 * trial + 3 * j + k) % len(n_obs)], 100 * k + 10 * trial + j),
                     n_ch[(3 * trial + 5 * j + k) % len(n_ch)]) for j in range(1 + (trial + k) % 6)]
            segs.append((gen(n_obs[(trial + k) % len(n_obs)], 7), 9))          # always ends on a draw
            _same(gpu.transcript(segs), oracle.transcript(segs), ("transcript", gname, trial, [(len(w), c) for w, c in segs]))


# ---- NTT / LDE ----------------------------------------------------------------------------------------------------------
_columns = ev.columns          # (shared with tests/test_gpu_high_rate_edge_values.py and the CPU twins)


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("log_n", [3, 6])
def test_lde_commit_vs_python_integers(gpu, log_n, from_coeffs):
    n = 1 << log_n
    cols = _columns(n, 200 + log_n)
    vals = np.stack(list(cols.values()))
    for rate_bits in (1, 2, 3):
        cg, lg, _cap = gpu.lde_commit(vals, rate_bits, 0, from_coeffs)
        for k, name in enumerate(cols):
            coeffs = vals[k] if from_coeffs else ev.intt_naive(vals[k])
            _same(cg[k], coeffs, ("coefficients", name, log_n, rate_bits))
            _same(lg[k], ev.coset_lde_naive(coeffs, rate_bits), ("lde", name, log_n, rate_bits))


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("log_n", [3, 6, 10, 11, 13, 16])        # kernels_ntt.hip: one pass up to log_n 10, two above
def test_lde_commit_vs_oracle_on_edge_columns(gpu, oracle, log_n, from_coeffs):
    n = 1 << log_n
    cols = _columns(n, 300 + log_n)
    vals = np.stack(list(cols.values()))
    for rate_bits in (1, 2, 3):
        cap_h = min(4, log_n + rate_bits)
        co, lo, capo = oracle.lde_commit(vals, rate_bits, cap_h, from_coeffs)
        cg, lg, capg = gpu.lde_commit(vals, rate_bits, cap_h, from_coeffs)
        what = (list(cols), log_n, rate_bits, from_coeffs)
        _same(cg, co, ("coefficients",) + what)
        _same(lg, lo, ("lde",) + what)
        _same(capg, capo, ("cap",) + what)


def test_full_size_lde_of_structured_columns(gpu):
    """BASELINE's shape (135 columns x 2^16, LDE 2^19), no oracle involved: closed forms.
    Values in: const(p-1) -> (p-1) delta(0), whose LDE is the constant p-1; delta(r, p-1) -> -(n^-1) w^(-rk);
    geometric(w^j) -> delta(j), whose LDE is (7 w_big^i)^j.  Coefficients in: c X^k -> c (7 w_big^i)^k."""
    log_n, rate, W = 16, 3, 135
    n, big = 1 << log_n, 1 << (log_n + rate)
    w = ev.root_of_unity(log_n)
    # (name, values, expected coefficients, expected LDE or None)
    patterns = [("const(p-1)", ev.const(n, P - 1), ev.intt_of_const(n, P - 1), ev.const(big, P - 1))]
    for r in (0, 1, n // 2, n - 1):
        patterns.append((f"delta({r},p-1)", ev.delta(n, r, P - 1), ev.intt_of_delta(n, r, P - 1), None))
    for j in (1, n // 2, n - 1):
        patterns.append((f"geometric(w^{j})", ev.geometric(n, pow(w, j, P)), ev.intt_of_geometric(n, j),
                         ev.lde_of_monomial(log_n + rate, 1, j)))
    vals = np.stack([patterns[k % len(patterns)][1] for k in range(W)])
    cg, lg, _cap = gpu.lde_commit(vals, rate, 4)
    for k in range(W):
        name, _v, coeffs, lde = patterns[k % len(patterns)]
        _same(cg[k], coeffs, ("coefficients", name, "column", k))
        if lde is not None:
            _same(lg[k], lde, ("lde", name, "column", k))
    assert (lg < PU).all()
    # coefficients in: one-coefficient polynomials c X^k
    monos = [(c, k) for k in (0, 1, n - 1) for c in (P - 1, EPS, 1)]
    want = [ev.lde_of_monomial(log_n + rate, c, k) for c, k in monos]
    vals = np.stack([ev.delta(n, monos[i % len(monos)][1], monos[i % len(monos)][0]) for i in range(W)])
    cg, lg, _cap = gpu.lde_commit(vals, rate, 4, from_coeffs=True)
    _same(cg, vals, "coefficients handed back")
    for i in range(W):
        _same(lg[i], want[i % len(monos)], ("lde of c X^k", monos[i % len(monos)], "column", i))


# ---- openings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 10, 16, 18])               # 18: the chunked form
def test_eval_polys_on_edge_coefficients(gpu, oracle, log_n):
    n = 1 << log_n
    coeffs = np.stack([ev.edge(n, 400 + log_n), ev.const(n, P - 1), ev.mixed(n, 410 + log_n), ev.delta(n, n - 1, P - 1)])
    points = ev.OPENING_POINTS + [(ev.root_of_unity(log_n), 0), (pow(ev.root_of_unity(log_n), 3, P), 0)]
    for pt in points:
        for scale in ev.OPENING_SCALES + [ev.root_of_unity(log_n)]:
            z = np.array(pt, dtype=np.uint64)
            _same(gpu.eval_polys(coeffs, z, scale), oracle.eval_polys(coeffs, z, scale), ("eval_polys", log_n, pt, scale))
    if log_n <= 10:                                             # and the Python form where it can go
        for pt, scale in ((ev.OPENING_POINTS[4], P - 1), (ev.OPENING_POINTS[3], 1)):
            got = gpu.eval_polys(coeffs, np.array(pt, dtype=np.uint64), scale)
            for k in range(coeffs.shape[0]):
                assert tuple(int(v) for v in got[k]) == ev.horner_ext(coeffs[k], pt, scale), (log_n, pt, scale, k)
    if log_n <= 16:
        # zeta = (7 w_big^i, 0): the answer is the LDE word, which the NTT tests pin
        rate = 3
        _c, lde, _cap = gpu.lde_commit(coeffs, rate, 0, from_coeffs=True)
        _same(lde, oracle.lde_commit(coeffs, rate, 0, True)[1], ("lde", log_n))
        w_big = ev.root_of_unity(log_n + rate)
        big = n << rate
        for i in (0, 1, big // 2, big - 1, 5 % big):
            x = 7 * pow(w_big, i, P) % P
            got = gpu.eval_polys(coeffs, np.array([x, 0], dtype=np.uint64))
            rev = ev.bit_reverse(i, log_n + rate)
            assert (got[:, 1] == 0).all() and (got[:, 0] == lde[:, rev]).all(), (log_n, i)


# ---- FRI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,rate_bits,cap_h,arity,pow_bits,queries", [       # test_fri_prove_vs_oracle's, less the largest
    (10, 3, 4, [4, 4], 8, 5),
    (12, 3, 4, [4, 4], 10, 28),
    (12, 3, 2, [4, 4, 4], 10, 9),
    (8, 1, 0, [3, 2, 1], 4, 7),
    (6, 2, 2, [], 6, 3),
])
def test_fri_prove_on_edge_polynomials(gpu, oracle, log_n, rate_bits, cap_h, arity, pow_bits, queries):
    seed = ev.uniform(13, 99)
    for name, coeffs in ev.fri_polynomials(log_n).items():
        g, st = gpu.fri_prove(coeffs, rate_bits, cap_h, arity, pow_bits, queries, seed)
        assert st == 0, name
        o = oracle.fri_prove(coeffs, rate_bits, cap_h, arity, pow_bits, queries, seed)      # asserts its own success
        _same(g, o, ("fri_prove", name, log_n))


# ---- partial products and quotient --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(gpu, oracle):
    return stage_circuits.build_small(gpu, oracle)


@pytest.fixture(scope="module")
def rec_small(gpu, oracle):
    return stage_circuits.build_rec_small(gpu, oracle)


def _check_a7_a8(c, oc, wires, betas, gammas, alphas, what):
    zo = oc.partial_products(wires, betas, gammas)
    # the condition of these tests, on the reference alone: no denominator w + beta * sigma + gamma is zero
    assert zo.all(), (what, "the oracle's zs_pp holds a zero: this input inverts zero and is outside the contract")
    _same(c.partial_products(wires, betas, gammas), zo, ("partial_products",) + what)
    _same(c.quotient(wires, zo, betas, gammas, alphas), oc.quotient(wires, zo, betas, gammas, alphas), ("quotient",) + what)
    return zo


def _whole_matrices(c, oc, wires, tag):
    betas, gammas, alphas = ev.uniform_challenges(11)
    _check_a7_a8(c, oc, wires, betas, gammas, alphas, (tag, "witness"))
    for name, w in ev.wire_matrices(wires.shape):
        zo = _check_a7_a8(c, oc, w, betas, gammas, alphas, (tag, name))
        if name == "edge":
            # zs_pp itself from the boundary list, fed to the quotient directly
            z = ev.edge(zo.size, 17).reshape(zo.shape)
            _same(c.quotient(w, z, betas, gammas, alphas), oc.quotient(w, z, betas, gammas, alphas),
                  ("quotient", tag, "edge wires, edge zs_pp"))
            _same(c.quotient(wires, z, betas, gammas, alphas), oc.quotient(wires, z, betas, gammas, alphas),
                  ("quotient", tag, "witness, edge zs_pp"))


def _boundary_challenges(c, oc, wires, tag, witness_too):
    edge_wires = dict(ev.wire_matrices(wires.shape))["edge"]
    for name, b, g, a in ev.boundary_challenge_cases():
        _check_a7_a8(c, oc, edge_wires, b, g, a, (tag, "edge wires", name))
        if witness_too:
            _check_a7_a8(c, oc, wires, b, g, a, (tag, "witness", name))


def _one_row_per_gate_kind(c, oc, wires, tag, want_kinds):
    """The satisfied witness with one row overwritten: a failure names the gate kind whose evaluator read the row."""
    rows = stage_circuits.first_row_of_each_kind(c.to_blob())
    assert set(want_kinds) <= set(rows), (sorted(rows), want_kinds)
    betas, gammas, alphas = ev.uniform_challenges(12)
    for kind, row in sorted(rows.items()):
        for k, (gname, gen) in enumerate(ev.GENERATORS.items()):
            w = wires.copy()
            w[:, row] = gen(wires.shape[0], 1000 * kind + k)
            _check_a7_a8(c, oc, w, betas, gammas, alphas, (tag, f"gate kind {kind} (row {row})", gname))


def test_stage_kernels_on_edge_wire_matrices_small(small):
    _whole_matrices(*small, "small")


def test_stage_kernels_under_boundary_challenges_small(small):
    _boundary_challenges(*small, "small", witness_too=True)


def test_stage_kernels_one_edge_row_per_gate_kind_small(small):
    _one_row_per_gate_kind(*small, "small", range(1, 11))


def test_stage_kernels_on_edge_wire_matrices_recursion(rec_small):
    _whole_matrices(*rec_small, "rec_small")


def test_stage_kernels_under_boundary_challenges_recursion(rec_small):
    _boundary_challenges(*rec_small, "rec_small", witness_too=False)


def test_stage_kernels_one_edge_row_per_gate_kind_recursion(rec_small):
    _one_row_per_gate_kind(*rec_small, "rec_small", range(11, 18))      # and the inner kinds it holds, on k_quotient_rec


def test_stage_kernels_on_mixed_wires_fib64(gpu, fib_circuit, fib_oracle):
    """Full size once: 2^16 rows x 135 wires, the shapes k_zpp_* and k_quotient run at in the benchmark."""
    n_wires, n = int(fib_circuit.info.num_wires), 1 << int(fib_circuit.info.degree_bits)
    wires = ev.mixed(n_wires * n, 77).reshape(n_wires, n)
    betas, gammas, alphas = ev.uniform_challenges(21)
    _check_a7_a8(fib_circuit, fib_oracle, wires, betas, gammas, alphas, ("fib64", "mixed"))


# ---- whole proofs: gadget circuits on boundary inputs (the part that reaches kernels_witgen.hip) ---------------------------
def _prove_and_compare(gpu, oracle, kind, param, inputs, what):
    c = gpu.Circuit.build_gadget(kind, param)
    oc = oracle.load_circuit(c.to_blob())
    batch = np.array(inputs, dtype=np.uint64).reshape(len(inputs), -1)
    seeds = list(range(21, 21 + len(inputs)))
    proofs, st = c.prove(batch, seeds=seeds)
    assert st.tolist() == [0] * len(inputs), (what, st.tolist())
    dg, cap = c.digest()
    for i in range(len(inputs)):
        wg, stw = c.witness(batch[i], seed=seeds[i])
        wo, sto, msg = oc.witness(batch[i], seed=seeds[i])
        assert stw == 0 and sto == 0, (what, i, msg)
        _same(wg, wo, (what, "witness", [hex(int(v)) for v in batch[i]][:8]))
        po, sto, _t, msg = oc.prove(batch[i], seed=seeds[i])
        assert sto == 0, (what, i, msg)
        _same(proofs[i], po, (what, "proof", [hex(int(v)) for v in batch[i]][:8]))
        assert oc.verify(proofs[i], dg, cap)[0] == 0, (what, i)
    return c, proofs


def test_prove_and_xor_on_boundary_words(gpu, oracle):
    words = [0, 0xFFFFFFFF, P - 1]
    pairs = [(x, y) for x in words for y in words]
    assert (0, 0) in pairs and (0xFFFFFFFF, 0xFFFFFFFF) in pairs and (0, 0xFFFFFFFF) in pairs
    _prove_and_compare(gpu, oracle, 0, 0, [[x, y, (x & y) % P] for x, y in pairs], "and")
    _prove_and_compare(gpu, oracle, 1, 0, [[x, y, (x ^ y) % P] for x, y in pairs], "xor")


def test_prove_poseidon2_compress_on_boundary_halves(gpu, oracle):
    halves = [(ev.const(4, P - 1), ev.const(4, P - 1)), (ev.edge(4, 1), ev.edge(4, 2)), (ev.const(4, 0), ev.const(4, P - 1)),
              (ev.high(4, 3), ev.low(4, 4)), (ev.edge(4, 5), ev.const(4, 0))]
    inputs = []
    for l, r in halves:
        state = np.concatenate([l, r, np.zeros(4, dtype=np.uint64)])
        out = oracle.poseidon2_permute(state)[0][:4]
        inputs.append([int(v) for v in l] + [int(v) for v in r] + [int(v) for v in out])
    _prove_and_compare(gpu, oracle, 5, 0, inputs, "compress")


def test_prove_connected_inputs_on_boundary_words(gpu, oracle):
    _prove_and_compare(gpu, oracle, 8, 0, [[a, a, a * a % P] for a in (0, 1, P - 1, EPS, P - EPS, 1 << 63)], "a*b, a = b")


def test_prove_public_input_products_of_edge_inputs(gpu, oracle):
    n = 9
    non_zero = [v for v in EDGE if v]
    inputs = [[int(v) for v in ev.edge(n, s)] for s in (1, 2)] + [non_zero[:n], non_zero[-n:], [P - 1] * n]
    c, proofs = _prove_and_compare(gpu, oracle, 11, n, inputs, "public inputs")
    for inp, proof in zip(inputs, proofs):
        pis = [int(v) for v in c.public_inputs(proof)]
        prod, want = inp[0], list(inp)
        for v in inp[1:]:
            prod = prod * v % P
            want.append(prod)
        assert pis == want, inp


def test_prove_extension_chain_on_boundary_operands(gpu, oracle):
    """Gadget 9: ((5 ((a b + c) a - b) + (3 + 9 X))^7 / c + a + b + a0 b in F_p^2, a and b from EDGE, c invertible; the
    expectation is computed here in Python integers and the oracle's witness generator must accept it."""
    def add(x, y):
        return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)

    inputs = []
    for a, b, cc in (((P - 1, P - 1), (P - 1, 0), (1, 0)), ((0, 0), (0, 0), (P - 1, P - 1)), ((EPS, P - EPS), (1 << 63, 1), (0, 1)),
                     ((P - 1, 0), (0, P - 1), (EPS, 0)), ((1, 0), (P - 2, EPS + 1), (P - EPS, P - 1)),
                     ((EDGE[5], 7), ((P - 1) // 2, (P + 1) // 2), (7, EDGE[5]))):
        t = add(ev.ext_mul(a, b), cc)
        t = add(ev.ext_mul(t, a), ((P - b[0]) % P, (P - b[1]) % P))
        t = add((5 * t[0] % P, 5 * t[1] % P), (3, 9))
        t7 = t
        for _ in range(6):
            t7 = ev.ext_mul(t7, t)
        q = ev.ext_mul(t7, ev.ext_inv(cc))
        s = add(add(add(q, a), b), (a[0] * b[0] % P, a[0] * b[1] % P))
        inputs.append(list(a) + list(b) + list(cc) + list(s))
    _prove_and_compare(gpu, oracle, 9, 0, inputs, "extension chain")


# ---- words >= p at the five primitive entry points ---------------------------------------------------------------------------
# include/p25.h: the rule per entry point.  "reduces": the kernels take any u64, the result is the result for the reduced
# words and is canonical.  "refuses": P25_ERR_INVALID_ARG, as the stage entry points answer.  Never a different
# canonical-looking answer.  The oracle is only ever given the reduced words.
def _with_noncanonical(words):
    """(raw, reduced): `words` with every fifth word replaced by one of NONCANONICAL."""
    raw = np.array(words, dtype=np.uint64).ravel().copy()
    for k, i in enumerate(range(0, raw.size, 5)):
        raw[i] = np.uint64(ev.NONCANONICAL[k % len(ev.NONCANONICAL)])
    reduced = np.array([int(v) % P for v in raw], dtype=np.uint64)
    assert (raw >= PU).any() and (reduced < PU).all()
    return raw, reduced


def _reduces_or_refuses(gpu, call, raw, want, what):
    """Outcome (a) or (b) of the contract; returns which."""
    try:
        got = call(raw)
    except gpu.P25Error as e:
        assert e.status == 1, (what, e)
        return "refuses"
    for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
        _same(g, w, (what, "on words >= p"))
    return "reduces"


NONCANONICAL_RULE = {"poseidon_permute": "reduces", "poseidon2_permute": "refuses", "merkle_commit": "refuses",
                     "lde_commit": "refuses", "transcript": "refuses"}


def test_noncanonical_words_poseidon_permute(gpu, oracle):
    raw, red = _with_noncanonical(ev.edge(12 * 64, 5))
    raw[:12], red[:12] = np.uint64(P), 0                                 # whole states of p and of 2^64 - 1
    raw[12:24], red[12:24] = np.uint64((1 << 64) - 1), EPS - 1
    got = _reduces_or_refuses(gpu, gpu.poseidon_permute, raw.reshape(-1, 12), oracle.poseidon_permute(red.reshape(-1, 12)),
                              "poseidon_permute")
    assert got == NONCANONICAL_RULE["poseidon_permute"]


def test_noncanonical_words_poseidon2_permute(gpu, oracle):
    raw, red = _with_noncanonical(ev.edge(12 * 64, 6))
    raw[:12], red[:12] = np.uint64(P), 0                                 # whole states of p and of 2^64 - 1
    raw[12:24], red[12:24] = np.uint64((1 << 64) - 1), EPS - 1
    got = _reduces_or_refuses(gpu, gpu.poseidon2_permute, raw.reshape(-1, 12), oracle.poseidon2_permute(red.reshape(-1, 12)),
                              "poseidon2_permute")
    assert got == NONCANONICAL_RULE["poseidon2_permute"]


@pytest.mark.parametrize("width", [3, 9, 135])                  # a leaf that is its own digest (its words would be tree words), k_hash_leaves, k_hash_leaves_wide
def test_noncanonical_words_merkle_commit(gpu, oracle, width):
    n = 64
    raw, red = _with_noncanonical(ev.edge(n * width, 8))
    raw, red = raw.reshape(n, width), red.reshape(n, width)
    want = oracle.merkle_commit(red, 2, want_tree=True)
    got = _reduces_or_refuses(gpu, lambda a: gpu.merkle_commit(np.ascontiguousarray(a.T), 2, want_tree=True), raw, want,
                              ("merkle_commit", width))
    assert got == NONCANONICAL_RULE["merkle_commit"]


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("log_n", [6, 11])
def test_noncanonical_words_lde_commit(gpu, oracle, log_n, from_coeffs):
    n = 1 << log_n
    raw, red = _with_noncanonical(ev.edge(3 * n, 9))
    raw, red = raw.reshape(3, n), red.reshape(3, n)
    want = oracle.lde_commit(red, 3, 2, from_coeffs)
    got = _reduces_or_refuses(gpu, lambda a: gpu.lde_commit(a, 3, 2, from_coeffs), raw, want, ("lde_commit", log_n, from_coeffs))
    assert got == NONCANONICAL_RULE["lde_commit"]


def test_noncanonical_words_transcript(gpu, oracle):
    outcomes = set()
    for n_obs in (1, 7, 8, 9, 100):
        raw, red = _with_noncanonical(ev.edge(n_obs, 10 + n_obs))
        want = oracle.transcript([(red, 5), (red[:3], 9)])
        outcomes.add(_reduces_or_refuses(gpu, lambda a: gpu.transcript([(a, 5), (a[:3], 9)]), raw, want, ("transcript", n_obs)))
    assert outcomes == {NONCANONICAL_RULE["transcript"]}
