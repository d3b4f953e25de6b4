"""GPU: the device prover at FRI rates 4..8, byte-equal to the oracle.

  LDE            2^rb cosets in one pass-1 launch (coset c stored as block rev(c)); the coset pre-scale unfactored while its
                 table stays within 2^19 words or the transform is a single pass, factored above that
  quotient       evaluated on the sub-coset of 8n points that the first 8n words of every LDE column are; the inverse
                 transform runs at degree_bits + 3
  whole proofs   gadget circuits (no FRI layer) and the 2^11-row shrink circuit (two layers, two-pass LDE), each as a lone
                 proof and as a batch of three: the batch takes the throughput launch forms
  shrink chain   (7, 12, 16) then (8, 10, 16) on the device end to end
  verifier       p25_verify_batch's verdicts at rates 5 and 8 against the oracle's

The oracle takes 20-30 s for a proof of the 2^11-row circuit at rate 8, so those three proofs are recorded
(tests/golden/high_rate/, tools/record_high_rate_golden.py; tests/test_high_rate_cpu.py holds them to the live oracle)."""
import os

import numpy as np
import pytest

import gadget_cases
import high_rate as hr
import verify_cases
from conftest import P, ROOT, splitmix_field
from verify_cases import INITIAL_MERKLE, OK, VANISHING, expected, flipped, reference_gates_inputs

pytestmark = pytest.mark.gpu

RATES = [(4, 21), (5, 17), (7, 12), (8, 10)]
GOLD = os.path.join(ROOT, "tests", "golden", "high_rate", "shrink_gadget8_rate8.npz")


# ---------------------------------------------------------------------------------------------------------------------
# LDE
# ---------------------------------------------------------------------------------------------------------------------
LDE_CASES = [(10, 3, 4), (10, 1, 8),     # single pass: 16 and 256 cosets
             (11, 3, 4), (11, 1, 8),     # smallest two-pass; 2^19 table words: the last unfactored size
             (12, 1, 8),                 # two-pass, 2^20 table words: factored at a small size
             (12, 1, 5), (13, 3, 6),     # radix remainders beside a radix-16 group
             (16, 1, 4),                 # the constant-shape instantiation (pass 2; pass 1 factored)
             (17, 1, 4)]                 # factored by size


@pytest.mark.parametrize("log_n,cols,rate", LDE_CASES)
def test_lde_commit_forms_vs_oracle(gpu, oracle, log_n, cols, rate):
    """From values and from coefficients; the oracle's coefficients of the first are the input of the second, whose LDE and
    cap are therefore the same (one oracle LDE per case: at 2^21 points it is what the case costs)."""
    n = 1 << log_n
    vals = splitmix_field(n * cols, seed=2100 + 16 * log_n + 4 * cols + rate).reshape(cols, n)
    co, lo, capo = oracle.lde_commit(vals, rate, 4, False)
    for from_coeffs, given in ((False, vals), (True, co)):
        cg, lg, capg = gpu.lde_commit(given, rate, 4, from_coeffs)
        what = (log_n, cols, rate, from_coeffs)
        assert (cg == co).all(), what
        assert lg.shape == lo.shape and (lg == lo).all(), (what, np.argwhere(lg != lo)[:5])
        assert (capg == capo).all(), what


def test_lde_prefix_is_the_rate_3_lde(gpu):
    """The layout identity the quotient kernel rests on: lde_rb[rev_{k+rb}(2^(rb-3) i)] = lde_3[rev_{k+3}(i)], i.e. the first
    8n words of a bit-reversed LDE column of any rate above 3 are the rate-3 column."""
    vals = splitmix_field(3 << 11, seed=77).reshape(3, 1 << 11)
    _c, l3, _cap = gpu.lde_commit(vals, 3, 4, True)
    for rate in (4, 6, 8):
        _c, lr, _cap = gpu.lde_commit(vals, rate, 4, True)
        assert (lr[:, :8 << 11] == l3).all(), rate


def test_lde_rates_and_sizes_refused(gpu, p25):
    vals = splitmix_field(1 << 6).reshape(1, 64)
    with pytest.raises(p25.P25Error):
        gpu.lde_commit(vals, 9, 4)
    big = np.zeros((1, 1 << 17), dtype=np.uint64)
    with pytest.raises(p25.P25Error):
        gpu.lde_commit(big, 8, 4)          # 17 + 8 = 25


# ---------------------------------------------------------------------------------------------------------------------
# FRI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,rate,arity", [(6, 8, [4]), (10, 5, [4, 4]), (12, 4, [4, 4])])
def test_fri_prove_vs_oracle(gpu, oracle, log_n, rate, arity):
    coeffs = splitmix_field(2 << log_n, seed=3000 + log_n).reshape(2, 1 << log_n)
    seed = splitmix_field(13, seed=98)
    g, st = gpu.fri_prove(coeffs, rate, 4, arity, 10, hr.QUERIES[rate], seed)
    assert st == 0
    o = oracle.fri_prove(coeffs, rate, 4, arity, 10, hr.QUERIES[rate], seed)
    assert g.shape == o.shape
    diff = np.nonzero(g != o)[0]
    assert diff.size == 0, f"first differing words {diff[:8]} of {g.size}"


# ---------------------------------------------------------------------------------------------------------------------
# the quotient stage
# ---------------------------------------------------------------------------------------------------------------------
def _quotient_parity(c, oc, wires, seed):
    betas, gammas, alphas = splitmix_field(6, seed=seed).reshape(3, 2)
    zg = c.partial_products(wires, betas, gammas)
    zo = oc.partial_products(wires, betas, gammas)
    assert (zg == zo).all()
    qg = c.quotient(wires, zg, betas, gammas, alphas)
    qo = oc.quotient(wires, zo, betas, gammas, alphas)
    assert qg.shape == qo.shape == (16, 1 << int(c.info.degree_bits)) and (qg == qo).all(), np.argwhere(qg != qo)[:5]
    assert qg.any()


@pytest.mark.parametrize("rate", [4, 8])
def test_quotient_stage_gadget_14(gpu, oracle, rate):
    c = gpu.Circuit.build_gadget(14, 0, (rate, hr.QUERIES[rate], 16))
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF), seed=4)
    assert st == 0, msg
    _quotient_parity(c, oc, wires, 40 + rate)
    c.close()


def test_quotient_stage_2_10_rows_at_rate_4(gpu, oracle):
    """The 2^10-row plonky3-verifier circuit rebuilt by blob rewrite to rate 4: a 2^13-point inverse transform from the
    prefix of 2^14-point LDE columns."""
    inp, cfg = gpu.p3_prove_fibonacci(3, 3, 4)
    std = gpu.Circuit.build_p3_verifier(cfg)
    c = gpu.Circuit.from_blob(hr.rewrite_config(std.to_blob(), 4, hr.QUERIES[4]))
    assert int(c.info.degree_bits) == 10 and c.config.as_tuple() == (4, 21, 16)
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(inp, seed=5)
    assert st == 0, msg
    _quotient_parity(c, oc, wires, 31)
    c.close()
    std.close()


# ---------------------------------------------------------------------------------------------------------------------
# whole proofs
# ---------------------------------------------------------------------------------------------------------------------
def _gadget_inputs(oracle, kind):
    if kind == 11:
        return 3, hr.public_inputs_gadget_inputs(3)
    if kind == 14:
        return 0, reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF)
    _name, _kind, param, inputs = [c for c in gadget_cases.cases() if c[1] == kind][0]
    return param, inputs


def _lone_and_batch(c, inputs, want, seeds=(0, 1, 2)):
    """Seed 0 as a lone proof, then all three in one batch: statuses and every proof word against `want`."""
    inp = np.asarray(inputs, dtype=np.uint64)
    lone, st = c.prove(inp[None, :], seeds=[seeds[0]])
    assert st.tolist() == [0]
    diff = np.nonzero(lone[0] != want[0])[0]
    assert diff.size == 0, f"lone proof: first differing words {diff[:8]} of {lone[0].size}"
    batch, st = c.prove(np.stack([inp] * len(seeds)), seeds=list(seeds))
    assert st.tolist() == [0] * len(seeds)
    for k in range(len(seeds)):
        diff = np.nonzero(batch[k] != want[k])[0]
        assert diff.size == 0, f"batch proof {k}: first differing words {diff[:8]} of {batch[k].size}"
    return batch


@pytest.mark.parametrize("rate,queries", RATES)
@pytest.mark.parametrize("kind", [9, 11, 14])
def test_gadget_proofs_equal_the_oracles(gpu, oracle, kind, rate, queries):
    param, inputs = _gadget_inputs(oracle, kind)
    c = gpu.Circuit.build_gadget(kind, param, (rate, queries, 16))
    oc = oracle.load_circuit(c.to_blob())
    assert int(c.info.proof_words) == oc.proof_words
    want = []
    for seed in (0, 1, 2):
        p, st, _tm, msg = oc.prove(np.asarray(inputs, dtype=np.uint64), seed=seed)
        assert st == 0, msg
        want.append(p)
    batch = _lone_and_batch(c, inputs, want)
    dg, cap = c.digest()
    assert oc.verify(batch[2], dg, cap)[0] == 0 and c.verify(batch).tolist() == [OK] * 3
    # a wrong expectation is a witness conflict on both sides, at any rate
    if kind == 9:
        bad = list(inputs)
        bad[-1] = (bad[-1] + 1) % P
        _p, st = c.prove(np.asarray(bad, dtype=np.uint64)[None, :], seeds=[0])
        assert st.tolist() == [4] and oc.prove(np.asarray(bad, dtype=np.uint64), seed=0)[1] == 4
    c.close()


@pytest.fixture(scope="module")
def gadget8(gpu, oracle):
    """Gadget 8 and the oracle's proof of it: what the shrink circuits verify."""
    _name, kind, param, inputs = [c for c in gadget_cases.cases() if c[1] == 8][0]
    inner = gpu.Circuit.build_gadget(kind, param)
    oc = oracle.load_circuit(inner.to_blob())
    proof, st, _tm, msg = oc.prove(np.asarray(inputs, dtype=np.uint64), seed=1)
    assert st == 0, msg
    return inner, oc, proof


def test_shrink_circuit_proofs_at_rate_4_equal_the_oracles(gpu, oracle, gadget8):
    inner, _oc, proof = gadget8
    c = inner.build_shrink((4, 21, 16))
    assert int(c.info.degree_bits) == 11
    so = oracle.load_circuit(c.to_blob())
    want, st, _per, _wall = so.prove_many(np.stack([proof] * 3), [0, 1, 2], threads=3)
    assert st.tolist() == [0, 0, 0]
    _lone_and_batch(c, proof, want)
    c.close()


def test_shrink_circuit_proofs_at_rate_8_equal_the_oracles(gpu, oracle, gadget8):
    """2^11 rows, an LDE of 2^19 points per column, against the oracle's recorded proofs."""
    inner, _oc, proof = gadget8
    gold = np.load(GOLD)
    assert int(gold["inner_seed"]) == 1 and (gold["inner_proof"] == proof).all() and gold["seeds"].tolist() == [0, 1, 2]
    c = inner.build_shrink((8, 10, 16))
    assert int(c.info.degree_bits) == 11 and int(c.info.proof_words) == gold["proofs"].shape[1]
    so = oracle.load_circuit(c.to_blob())
    dg, cap = c.digest()
    odg, ocap = so.digest()
    assert (dg == odg).all() and (cap == ocap).all()
    batch = _lone_and_batch(c, proof, gold["proofs"])
    assert so.verify(batch[1], dg, cap)[0] == 0
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# the shrink chain
# ---------------------------------------------------------------------------------------------------------------------
def test_two_step_shrink_chain_on_the_device(gpu, oracle):
    inner = gpu.Circuit.build_gadget(11, 3)
    xs = hr.public_inputs_gadget_inputs(3)
    proofs, st = inner.prove(np.asarray(xs, dtype=np.uint64)[None, :], seeds=[1])
    assert st.tolist() == [0]
    pis = inner.public_inputs(proofs[0])
    assert pis.size == 5
    std = inner.build_shrink()
    circuits, out = gpu.aggregate.shrink(inner, proofs[0], hr.SHRINK_CHAIN)
    assert [c.config.as_tuple() for c in circuits] == list(hr.SHRINK_CHAIN)
    words = [int(std.info.proof_words)] + [int(c.info.proof_words) for c in circuits]
    assert words[0] > words[1] > words[2] and [p.size for p in out] == words[1:]
    for c, p in zip(circuits, out):
        assert c.public_inputs(p).tolist() == pis.tolist()
        assert c.verify(p[None, :]).tolist() == [OK]
        dg, cap = c.digest()
        so = oracle.load_circuit(c.to_blob())
        assert so.verify(p, dg, cap)[0] == 0
        assert c.verify(flipped(p, p.size - 1)[None, :]).tolist() == [expected(so, flipped(p, p.size - 1), dg, cap)] != [OK]
    # a false inner proof has no witness in the first step
    bad = proofs[0].copy()
    bad[70] ^= np.uint64(1)
    _p, st = circuits[0].prove(bad[None, :], seeds=[0])
    assert st.tolist() == [4]
    for c in circuits + [std, inner]:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# the verifier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,queries", [(5, 17), (8, 10)])
def test_verify_batch_verdicts_equal_the_oracles(gpu, oracle, monkeypatch, rate, queries):
    """Bit 0 of one word flipped per proof: every third word ahead of the first query round, every 97th behind it (the
    positions of tests/test_gpu_verify.py's gadget case), at the rate's own layout."""
    monkeypatch.setattr(verify_cases, "RATE_BITS", rate)
    monkeypatch.setattr(verify_cases, "NUM_QUERIES", queries)
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    c = gpu.Circuit.build_gadget(0, 0, (rate, queries, 16))
    oc = oracle.load_circuit(c.to_blob())
    proofs, st = c.prove(np.asarray([x, y, (x & y) % P], dtype=np.uint64)[None, :], seeds=[5])
    assert st.tolist() == [0]
    proof, (dg, cap) = proofs[0], c.digest()
    L = verify_cases.Layout(c)
    assert L.n_layers == 0 and L.total == proof.size and L.lde_bits == int(c.info.degree_bits) + rate
    words = list(range(0, L.queries, 3)) + list(range(L.queries, proof.size, 97))
    batch = np.stack([proof] + [flipped(proof, w) for w in words])
    got = c.verify(batch)
    want = np.array([expected(oc, p, dg, cap) for p in batch], dtype=np.int32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]]
    assert want[0] == OK and (want[1:] != OK).all() and {VANISHING, INITIAL_MERKLE} <= set(want[1:].tolist())
    c.close()
