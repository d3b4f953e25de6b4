"""The Python-integer models of the gate constraints (tests/gate_models.py) and of the partial products and quotient
(tests/quotient_model.py) against the oracle's C++ evaluators, on the host: per row and per circuit, at the standard
configuration and at others.  The models are the yardstick of tests/test_gpu_quotient_model.py; this file shows that they and
the oracle, written apart, agree -- and pins the models on the reference's own test vectors."""
import hashlib

import numpy as np
import pytest

import blob_writer as bw
import edge_values as ev
import gate_models as gm
import quotient_cases as qc
import quotient_model as qm
import reference_vectors as rv
import verify_cases as vc
import witgen_cases as wc
from conftest import P

STANDARD = (bw.NUM_WIRES, bw.NUM_ROUTED, 3)

# sha256 (first 16 hex digits) of the blobs MiniCircuit wrote before it had a configuration
BLOB_PINS = {
    "connected_inputs_product": "677d7943fe57ea30", "sum_of_products(3)": "1ff94472345d7fde",
    "reference_gates": "20cdebba34041a2a", "arithmetic": "744bccbd0e468ae6", "mul_extension": "9e1fc0d16d5b0be6",
    "arithmetic_extension": "8b76286d4b57cda9", "quotient_extension": "4502d93b4de29ba8", "low_high": "3336fd13e5e79357",
    "reverse_bits": "aa0e672a742add07", "exponentiation": "f618ca8dc9f895b7", "u32_arithmetic": "2284a6f24df8e9e4",
    "u32_bits": "bdf9c3f9db133113", "poseidon2": "11c835f1e88e639c", "poseidon": "3224a04118772979",
    "mixed_poseidon": "1ec43822716cde0c", "poseidon_mds": "9262c5555e8ad4f7", "random_access": "34afed3c0c793f1d",
    "reducing": "59e7cfcda45d2eba", "reducing_extension": "e1fba6000b3c3794", "coset_interpolation": "0ddfbb4168252944",
}


def test_default_configuration_writes_the_same_blobs():
    blobs = {"connected_inputs_product": bw.connected_inputs_product().to_blob(), "sum_of_products(3)": bw.sum_of_products(3).to_blob(),
             "reference_gates": bw.reference_gates().to_blob()}
    blobs.update({n: c.blob for n, c in wc.all_cases().items()})
    assert {n: hashlib.sha256(b).hexdigest()[:16] for n, b in blobs.items()} == BLOB_PINS
    explicit = wc.arithmetic_case(num_wires=135, num_routed=80, rate_bits=3)
    assert explicit.blob == wc.all_cases()["arithmetic"].blob


# ---- per row ------------------------------------------------------------------------------------------------------------------
def _model_row(kind, wires, consts, pih, base):
    """gate_models on one row in the oracle's shapes: wires [W][2], consts [2][2], pih [4] -> [(a, b)]."""
    if base:
        out = gm.constraints(kind, gm.Base, [int(w[0]) for w in wires], int(consts[0][0]), int(consts[1][0]), [int(v) for v in pih])
        return [(v, 0) for v in out]
    return gm.constraints(kind, gm.Ext, [(int(w[0]), int(w[1])) for w in wires], (int(consts[0][0]), int(consts[0][1])),
                          (int(consts[1][0]), int(consts[1][1])), [(int(v), 0) for v in pih])


def _oracle_row(oracle, kind, wires, consts, pih, base):
    return [(int(a), int(b)) for a, b in oracle.eval_gate(kind, wires, consts, pih, base=base)]


def _arbitrary_rows(kind):
    """(wires [135][2], consts [2][2], pih [4]): rows of EDGE operands in the pattern of edge_rows (every ordered pair of EDGE
    meets in the first columns over the rows taken), and edge / mixed / high fills."""
    u64 = lambda v: np.array(v, dtype=np.uint64)   # noqa: E731
    rows = wc.edge_rows(270 + 8, i_range=(kind % wc.L, (kind + 7) % wc.L), j_range=(1, 12))
    out = [(u64(r[:270]).reshape(135, 2), u64(r[270:274]).reshape(2, 2), u64(r[274:278])) for r in rows]
    for k, gen in enumerate((ev.edge, ev.mixed, ev.high)):
        out.append((gen(270, 500 + 10 * kind + k).reshape(135, 2), gen(4, 600 + kind + k).reshape(2, 2), gen(4, 700 + kind + k)))
    return out


@pytest.mark.parametrize("kind", gm.KINDS)
def test_gate_model_equals_oracle_on_arbitrary_rows(oracle, kind):
    for wires, consts, pih in _arbitrary_rows(kind):
        for base in (True, False):
            m = _model_row(kind, wires, consts, pih, base)
            assert len(m) == bw.GATE_CONSTRAINTS[kind]
            assert m == _oracle_row(oracle, kind, wires, consts, pih, base), (kind, base)


@pytest.fixture(scope="module")
def witnesses(oracle):
    """name -> (Circuit, oracle circuit, satisfied witness of operand row 0 and of the last operand row)."""
    out = {}
    for name in wc.NAMES:
        c = qc.circuit(name)
        oc = oracle.load_circuit(c.blob)
        ws = []
        for row in (0, len(c.case.rows) - 1):
            wires, st, msg = oc.witness(c.case.inputs(c.case.rows[row]), seed=3 + row)
            assert st == 0, (name, msg)
            ws.append(wires)
        out[name] = (c, oc, ws)
    return out


def test_satisfied_rows_give_zeros_in_model_and_oracle(oracle, witnesses):
    seen = set()
    for name, (c, _oc, ws) in witnesses.items():
        for wires in ws:
            pih = wires[:4, c.b["pi_row"]]
            for r, (kind, k0, k1) in enumerate(c.b["rows"]):
                row = np.stack([wires[:, r], np.zeros(135, dtype=np.uint64)], axis=1)
                consts = np.array([[k0, 0], [k1, 0]], dtype=np.uint64)
                for base in (True, False):
                    m = _model_row(kind, row, consts, pih, base)
                    assert m == [(0, 0)] * bw.GATE_CONSTRAINTS[kind], (name, r, kind)
                    assert m == _oracle_row(oracle, kind, row, consts, pih, base)
                seen.add(kind)
    assert seen == set(gm.KINDS)


@pytest.mark.parametrize("kind", gm.KINDS)
def test_model_depends_on_everything_reads_names_and_on_nothing_else(kind):
    """Guards the model against ignoring an input: each wire, constant and hash word of reads(kind), bumped alone, changes a
    constraint; a column outside reads(kind) changes none."""
    wires = [int(v) for v in ev.uniform(135, 800 + kind)]
    k, pih = [int(v) for v in ev.uniform(2, 801 + kind)], [int(v) for v in ev.uniform(4, 802 + kind)]
    if kind == bw.G_EXPONENTIATION:        # the base (wire 0) enters through bit * base: keep the bits from being all zero
        assert any(wires[1:67])
    base = gm.constraints(kind, gm.Base, wires, k[0], k[1], pih)
    rd = gm.reads(kind)
    for col in range(135):
        bumped = list(wires)
        bumped[col] = (bumped[col] + qc.bump_delta(col)) % P
        assert (gm.constraints(kind, gm.Base, bumped, k[0], k[1], pih) != base) == (col in rd["wires"]), (kind, col)
    for i in range(2):
        kk = list(k)
        kk[i] = (kk[i] + 1) % P
        assert (gm.constraints(kind, gm.Base, wires, kk[0], kk[1], pih) != base) == (i in rd["consts"]), (kind, i)
    for i in range(4):
        hh = list(pih)
        hh[i] = (hh[i] + 1) % P
        assert (gm.constraints(kind, gm.Base, wires, k[0], k[1], hh) != base) == rd["pi"], (kind, i)


def test_models_reproduce_the_reference_gates_own_vectors():
    """U32ArithmeticGate on the wires of the reference's `get_wires`: 108 zeros on every satisfied row; under the non-canonical
    addend exactly p - 1 at the three (hi_not_max * low) positions and zero elsewhere."""
    for name, wires, satisfied in rv.u32_arithmetic_cases():
        w = [int(v) for v in wires] + [0] * (135 - len(wires))
        for F, lift in ((gm.Base, lambda v: v), (gm.Ext, lambda v: (v, 0))):
            out = gm.constraints(bw.G_U32_ARITHMETIC, F, [lift(v) for v in w], lift(0), lift(0), [lift(0)] * 4)
            assert len(out) == 108
            want = [lift(0)] * 108
            if not satisfied:
                for op in range(3):
                    want[36 * op] = lift(P - 1)
            assert out == want, name
    # the interleave vectors: a row holding the reference's operand, its bits and its expected output is satisfied
    bits = [(rv.INTERLEAVE_X >> (31 - b)) & 1 for b in range(32)]
    w = [rv.INTERLEAVE_X, rv.INTERLEAVE_EXPECTED, 0, 0, 0, 0] + bits + [0] * (135 - 38)
    assert gm.constraints(bw.G_U32_INTERLEAVE, gm.Base, w, 0, 0, [0] * 4) == [0] * 102
    bits = [(rv.UNINTERLEAVE_X >> (63 - b)) & 1 for b in range(64)]
    w = [rv.UNINTERLEAVE_X, rv.UNINTERLEAVE_EVENS_EXPECTED, rv.UNINTERLEAVE_ODDS_EXPECTED, 0, 0, 0] + bits + [0] * (135 - 70)
    assert gm.constraints(bw.G_U32_UNINTERLEAVE, gm.Base, w, 0, 0, [0] * 4) == [0] * 134
    # Poseidon2Gate's wire pins: the columns the model reads the swap, a delta and an output from
    pins = rv.POSEIDON2_WIRE_PINS
    w = [int(v) for v in ev.uniform(135, 9)]
    base = gm.constraints(bw.G_POSEIDON2, gm.Base, w, 0, 0, [0] * 4)
    for pin, changed in ((pins["WIRE_SWAP"], 0), (pins["wire_delta(3)"], 4), (pins["wire_output(11)"], 122)):
        v = list(w)
        v[pin] = (v[pin] + 1) % P
        out = gm.constraints(bw.G_POSEIDON2, gm.Base, v, 0, 0, [0] * 4)
        assert out[changed] != base[changed]


# ---- whole circuits -----------------------------------------------------------------------------------------------------------
def _check_circuit(c, oc, witness):
    """Model == oracle for the partial products and the quotient on every data set of `c`."""
    for label, wires, betas, gammas, alphas in qc.data_sets(c, witness):
        zs, q = qc.model(c, label, wires, betas, gammas, alphas)        # raises on a zero denominator
        assert np.array_equal(zs, oc.partial_products(wires, betas, gammas)), (c.key, label)
        qo = oc.quotient(wires, zs, betas, gammas, alphas)
        assert q.shape == qo.shape and np.array_equal(q, qo), (c.key, label, np.argwhere(q != qo)[:4])
        assert q.any()
        if label == "witness":
            # deg(vanishing polynomial) <= 9 (n - 1) -- Z times eight linear factors of degree n - 1; the selector groups hold
            # the filtered gate constraints to the same bound -- so the quotient's is <= 8 n - 9: its top 8 words are zero
            for a in range(2):
                assert not q[8 * a + 7, c.n - 8:].any(), (c.key, a)


@pytest.mark.parametrize("name", wc.NAMES)
def test_quotient_model_equals_oracle(witnesses, name):
    c, oc, ws = witnesses[name]
    _check_circuit(c, oc, ws[0])


@pytest.mark.parametrize("name", qc.TWINS)
def test_quotient_model_equals_oracle_on_the_twin_with_a_poseidon_mds_row(oracle, name):
    c = qc.circuit(name, twin=True)
    assert bw.G_POSEIDON_MDS in c.b["kinds"] and set(c.case.gates) <= set(c.b["kinds"])
    oc = oracle.load_circuit(c.blob)
    wires, st, msg = oc.witness(c.inputs(), seed=5)
    assert st == 0, msg
    _check_circuit(c, oc, wires)


CONFIG_PAIRS = [(cfg, name) for cfg in qc.CONFIGS for name in qc.CONFIG_CASES + (qc.SUB_CASES[1:] if cfg[2] != 3 else [])]


@pytest.mark.parametrize("config,name", CONFIG_PAIRS, ids=["w%d-r%d-rate%d-%s" % (cfg + (name,)) for cfg, name in CONFIG_PAIRS])
def test_other_configurations_import_and_model_equals_oracle(p25, oracle, config, name):
    """Blobs with other wire counts, routed counts and rate: the library imports them, the oracle proves and verifies with
    them, and its partial products (NP = 7, 10 with a ragged last chunk, 15) and quotient are the model's."""
    c = qc.circuit(name, config)
    assert bw.G_PUBLIC_INPUT in c.b["kinds"]
    lib = p25.Circuit.from_blob(c.blob)
    info = lib.info
    assert (int(info.num_wires), int(info.num_routed_wires)) == config[:2]
    assert int(info.num_partial_products) == -(-config[1] // 8) - 1 and int(info.quotient_degree_factor) == 8
    lib.close()
    oc = oracle.load_circuit(c.blob)
    inp = c.inputs()
    wires, st, msg = oc.witness(inp, seed=5)
    assert st == 0, msg
    _check_circuit(c, oc, wires)
    proof, st, _t, msg = oc.prove(inp, seed=7)
    assert st == 0, msg
    assert oc.verify(proof)[0] == 0


@pytest.mark.parametrize("label,config,name,message", qc.REFUSED, ids=[r[0] for r in qc.REFUSED])
def test_configurations_the_library_refuses(p25, label, config, name, message):
    blob = qc.BUILDER[name](**dict(zip(("num_wires", "num_routed", "rate_bits", "num_constants"), config))).blob
    with pytest.raises(p25.P25Error) as e:
        p25.Circuit.from_blob(blob)
    assert e.value.status == 1 and message in str(e.value)


# ---- the identity at zeta, in F_p^2 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_extension_models_hold_the_identity_at_zeta_of_an_oracle_proof(p25, oracle, witnesses, name):
    """gate_models over F_p^2 and quotient_model.vanishing_terms on the openings of the oracle's proof: the two sides of
    Z_H(zeta) sum_k zeta^(n k) q_k(zeta) = sum_j alpha^j term_j(zeta) agree for both alphas, and no longer once one opened
    wire the circuit's gates read is changed."""
    c, oc, _ws = witnesses[name]
    lib = p25.Circuit.from_blob(c.blob)
    lay = vc.Layout(lib)
    proof, st, _t, msg = oc.prove(c.inputs(), seed=9)
    assert st == 0, msg
    dg, _cap = oc.digest()
    sides = qc.zeta_identity(oracle, lay, c.b, proof, dg)
    assert all(lhs == rhs for lhs, rhs in sides) and any(lhs != (0, 0) for lhs, _ in sides), sides
    kind = max(c.case.gates)
    bad = proof.copy()
    bad[lay.wires + 2 * gm.reads(kind)["wires"][-1]] ^= np.uint64(1)
    assert all(lhs != rhs for lhs, rhs in qc.zeta_identity(oracle, lay, c.b, bad, dg))
    lib.close()
