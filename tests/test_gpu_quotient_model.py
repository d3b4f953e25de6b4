"""GPU: the quotient and partial-product kernels (kernels_quotient.hip, kernels_zpp.hip) and the verifier's evaluators at zeta
(ext_gates.h behind k_verify_vanishing) against the Python-integer models of tests/gate_models.py and tests/quotient_model.py
-- not the oracle, which tests/test_quotient_model_cpu.py holds to the same models on the host.

Circuits, fills and challenges are tests/quotient_cases.py's, the same sets the CPU file runs (it asserts that none of them
meets a zero denominator).  Every comparison is np.array_equal with the model; every output word is asserted canonical.
No circuit has more than 2^6 rows, so one stage call is at most 512 points.
"""
import numpy as np
import pytest

import blob_writer as bw
import gate_models as gm
import quotient_cases as qc
import quotient_model as qm
import verify_cases as vc
import witgen_cases as wc
from conftest import P

pytestmark = pytest.mark.gpu
PU = np.uint64(P)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got < PU).all(), (what, "non-canonical word at", np.argwhere(got >= PU)[:5].tolist())
    assert np.array_equal(got, want), (what, "first differing words", np.argwhere(got != want)[:5].tolist())


@pytest.fixture(scope="module")
def device(gpu):
    """Circuit of quotient_cases -> the imported device circuit, each imported once."""
    made = {}

    def get(c):
        if c.key not in made:
            made[c.key] = gpu.Circuit.from_blob(c.blob)
        return made[c.key]

    return get


def _witness(dc, c):
    wires, st = dc.witness(c.inputs(), seed=qc.WITNESS_SEED)
    assert st == 0, c.key
    return wires


def _check_stages(dc, c, boundary=True):
    """p25_partial_products and p25_quotient == the model on every data set of `c` (the satisfied witness first)."""
    info = dc.info
    assert (int(info.num_wires), int(info.num_routed_wires)) == c.config[:2] and (1 << int(info.degree_bits)) == c.n
    for label, wires, betas, gammas, alphas in qc.data_sets(c, _witness(dc, c), boundary):
        zs, q = qc.model(c, label, wires, betas, gammas, alphas)
        _same(dc.partial_products(wires, betas, gammas), zs, (c.key, label, "partial products"))
        _same(dc.quotient(wires, zs, betas, gammas, alphas), q, (c.key, label, "quotient"))
        assert q.any()


# ---- a. every case at the standard configuration --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_stages_equal_the_model_on_every_case(device, name):
    """Kinds 11 to 17 run in k_quotient_rec, the others in k_quotient; together the seventeen circuits hold all 18 kinds."""
    c = qc.circuit(name)
    _check_stages(device(c), c)


def test_the_cases_hold_every_gate_kind():
    assert {k for n in wc.NAMES for k in qc.circuit(n).b["kinds"]} == set(gm.KINDS)


@pytest.mark.parametrize("name", qc.TWINS)
def test_stages_equal_the_model_on_the_twin_with_a_poseidon_mds_row(device, name):
    """The evaluators of the kinds below 11 inside quotient_body<true, ..>: the same circuit with one PoseidonMds row."""
    c = qc.circuit(name, twin=True)
    assert bw.G_POSEIDON_MDS in c.b["kinds"] and set(c.case.gates) <= set(c.b["kinds"])
    _check_stages(device(c), c)


# ---- b. every wire of every gate -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,part", qc.bump_parts())
def test_quotient_sees_every_wire_of_every_gate_as_the_model_does(device, kind, part):
    """One row of gate `kind` in a 2^2-row circuit under the edge fill: every wire the gate reads bumped in turn by a
    boundary delta, the device's quotient == the model's each time (and != the quotient before the bump)."""
    c, row = qc.gate_row_circuit(kind)
    dc = device(c)
    label, wires, betas, gammas, alphas = qc.data_sets(c)[0]
    assert label == "edge" and c.b["rows"][row][0] == kind and c.n == 4
    zs, base = qc.model(c, label, wires, betas, gammas, alphas)
    cols = gm.reads(kind)["wires"][part * qc.BUMP_PART:(part + 1) * qc.BUMP_PART]
    assert cols or kind == bw.G_NOOP
    for col in cols:
        bumped = wires.copy()
        bumped[col, row] = (int(bumped[col, row]) + qc.bump_delta(col)) % P
        want = qc.to_u64(qm.quotient(c.b, bumped, zs, betas, gammas, alphas))
        assert not np.array_equal(want, base), (kind, col)
        _same(dc.quotient(bumped, zs, betas, gammas, alphas), want, (kind, row, col))
    _same(dc.quotient(wires, zs, betas, gammas, alphas), base, (kind, row, "unbumped"))


# ---- c, d. other configurations; the _sub kernels ----------------------------------------------------------------------------
def _prove_three(oracle, dc, c):
    """A batch of 3: the proofs are the oracle's bytes, the device verifier and the oracle's accept them."""
    rows = [0, len(c.case.rows) // 2, len(c.case.rows) - 1]
    inp = np.stack([c.inputs(r) for r in rows])
    proofs, st = dc.prove(inp, seeds=[21, 22, 23])
    assert st.tolist() == [0, 0, 0], (c.key, st.tolist())
    oc = oracle.load_circuit(c.blob)
    dg, cap = dc.digest()
    for k in range(3):
        po, sto, _t, msg = oc.prove(inp[k], seed=21 + k)
        assert sto == 0, msg
        _same(proofs[k], po, (c.key, "proof", k))
        assert oc.verify(proofs[k], dg, cap)[0] == 0, (c.key, k)
    assert dc.verify(proofs).tolist() == [0, 0, 0], c.key


RATE3 = [(cfg, name) for cfg in qc.CONFIGS if cfg[2] == 3 for name in qc.CONFIG_CASES]


@pytest.mark.parametrize("config,name", RATE3, ids=["w%d-r%d-rate%d-%s" % (cfg + (name,)) for cfg, name in RATE3])
def test_other_wire_and_routed_counts(device, oracle, config, name):
    """num_routed 64, 84 and 128 (k_zpp_* and the permutation pass at NP = 7, 10 with a last chunk of 4 wires, and 15; the
    stand-alone gate_constant, gate_public_input, gate_arithmetic, gate_base_sum (low_high) and gate_mul_ext (mul_extension,
    quotient_extension) of quotient_body's general path); num_wires 80 and 200 beside the standard 80 routed."""
    c = qc.circuit(name, config)
    dc = device(c)
    assert int(dc.info.num_partial_products) == -(-config[1] // 8) - 1
    _check_stages(dc, c)
    _prove_three(oracle, dc, c)


RATE4 = [(cfg, name) for cfg in qc.CONFIGS if cfg[2] != 3 for name in qc.SUB_CASES]


@pytest.mark.parametrize("config,name", RATE4, ids=["w%d-r%d-rate%d-%s" % (cfg + (name,)) for cfg, name in RATE4])
def test_sub_coset_kernels_at_a_higher_rate(device, oracle, config, name):
    """rate_bits 4: k_quotient_sub (arithmetic) and k_quotient_rec_sub (reducing_extension) read every second point of the
    rate-4 LDE; the quotient is the model's, which knows the rate-3 coset alone."""
    c = qc.circuit(name, config)
    dc = device(c)
    assert int(dc.config.rate_bits) == 4 and int(dc.info.quotient_degree_factor) == 8
    _check_stages(dc, c)
    _prove_three(oracle, dc, c)


@pytest.mark.parametrize("label,config,name,message", qc.REFUSED, ids=[r[0] for r in qc.REFUSED])
def test_refused_configurations_stay_refused_with_a_device(gpu, label, config, name, message):
    blob = qc.BUILDER[name](**dict(zip(("num_wires", "num_routed", "rate_bits", "num_constants"), config))).blob
    with pytest.raises(gpu.P25Error) as e:
        gpu.Circuit.from_blob(blob)
    assert e.value.status == 1 and message in str(e.value)


# ---- e. the identity at zeta from a device proof ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_identity_at_zeta_of_a_device_proof_holds_in_the_model(device, oracle, name):
    """The openings of a device proof satisfy the model's identity at zeta over F_p^2 for both alphas, and p25_verify_batch
    accepts it: what k_verify_vanishing computed there is the model's value.  With one opened wire the gates read flipped,
    the model's identity fails and the device verifier rejects."""
    c = qc.circuit(name)
    dc = device(c)
    lay = vc.Layout(dc)
    proofs, st = dc.prove(c.inputs()[None, :], seeds=[9])
    assert st.tolist() == [0]
    dg, _cap = dc.digest()
    sides = qc.zeta_identity(oracle, lay, c.b, proofs[0], dg)
    assert all(lhs == rhs for lhs, rhs in sides) and any(lhs != (0, 0) for lhs, _ in sides), sides
    bad = proofs[0].copy()
    bad[lay.wires + 2 * gm.reads(max(c.case.gates))["wires"][-1]] ^= np.uint64(1)
    assert all(lhs != rhs for lhs, rhs in qc.zeta_identity(oracle, lay, c.b, bad, dg))
    assert dc.verify(np.stack([proofs[0], bad])).tolist() == [0, vc.VANISHING]
