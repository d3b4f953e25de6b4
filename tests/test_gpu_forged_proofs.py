"""GPU: the batch verifier and the device witness generator on proofs that fail exactly ONE check.

A flipped word of a finished proof (tests/test_gpu_verify.py) is caught by the vanishing identity, the PoW or an initial
Merkle path, because it moves the transcript.  The proofs here are forged by the oracle's forging prover
(tests/forged_proofs.py, oracle/ref_prover.h RFault): tampered with mid-proof and finished honestly, they pass every
check ahead of the targeted one.  They are what reaches the comparisons no flipped word reaches: openings against
commitments (the first FRI_EVAL, or FINAL_POLY without layers), a layer against the fold before it, the final polynomial
-- in `fri_lane`, in `verdict_lane`'s step mapping, in the kernels' key merge, and in the in-circuit verifier as the
device witness generator runs it.

The expected codes are the table's, written down from the documented order of checks; the oracle must agree with each.
Shapes: the `and` gadget (2^4 rows, no FRI layer) and its recursive verifier (2^11 rows, two FRI layers)."""
import numpy as np
import pytest

import forged_proofs as fp
from conftest import P
from device_buffers import Banded, Banded32, strided_rows
from verify_cases import FINAL_POLY, FRI_EVAL, FRI_MERKLE, INITIAL_MERKLE, MALFORMED, OK, Layout, expected, flipped

pytestmark = pytest.mark.gpu
WITNESS_CONFLICT = 4


class Case:
    """A circuit, the oracle's honest proof of it and the forged set, made once."""

    def __init__(self, oracle, c, inputs, seed):
        self.c, self.oc, self.inputs = c, oracle.load_circuit(c.to_blob()), np.asarray(inputs, dtype=np.uint64)
        self.proof, st, _t, msg = self.oc.prove(self.inputs, seed=seed)
        assert st == 0, msg
        self.dg, self.cap = c.digest()
        self.L, self.pw = Layout(c), int(c.info.proof_words)
        self.forged = fp.forge(self.oc, c, self.inputs)
        # the table and the oracle agree before any kernel is asked (for fri_layer1_half this is the condition on the seed)
        assert fp.oracle_codes(self.oc, self.forged, self.dg, self.cap) == [f.code for f in self.forged]

    def named(self, name):
        return next(f for f in self.forged if f.name == name)

    def same_as_oracle(self, proofs, want):
        got = self.c.verify(np.stack(proofs)).tolist()
        assert [expected(self.oc, p, self.dg, self.cap) for p in proofs] == want
        assert got == want


@pytest.fixture(scope="module")
def flat(gpu, oracle):
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    return Case(oracle, gpu.Circuit.build_gadget(0, 0), [x, y, (x & y) % P], fp.SEEDS["flat"])


@pytest.fixture(scope="module")
def layers(gpu, oracle, flat):
    case = Case(oracle, flat.c.build_recursive_verifier(1), flat.proof, fp.SEEDS["layers"])
    assert int(case.c.info.degree_bits) == 11 and case.L.n_layers == 2 and case.pw == 15189
    return case


@pytest.fixture(scope="module", params=["flat", "layers"])
def case(request):
    return request.getfixturevalue(request.param)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the batch verifier, host and device form
# ---------------------------------------------------------------------------------------------------------------------
def test_verify_batch_answers_forged_proofs_with_the_tables_codes(case):
    batch, want, names = fp.mixed(case.forged, case.proof, seed=21)
    got = case.c.verify(batch).tolist()
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert FINAL_POLY in want and OK in want and (FRI_EVAL in want) == (case.L.n_layers > 0)


def test_verify_batch_dev_on_banded_strided_buffers(case):
    batch, want, names = fp.mixed(case.forged, case.proof, seed=22)
    n, stride = len(want), case.pw + 3
    rows = np.full((n, stride), (1 << 64) - 1, dtype=np.uint64)               # poisoned padding behind every proof
    rows[:, :case.pw] = batch
    d_proofs, d_status = Banded(n * stride, before=4097), Banded32(n, before=4099)
    d_proofs.set(rows)
    case.c.verify_dev(d_proofs.ptr, n, stride, d_status.ptr)
    case.c.sync()
    got = d_status.get().tolist()
    assert got == want, [(n_, g, w) for n_, g, w in zip(names, got, want) if g != w]
    d_status.assert_bands_intact()
    d_proofs.assert_unchanged()
    _data, pad = strided_rows(n, case.pw, stride)
    assert (d_proofs.get()[pad] == np.uint64((1 << 64) - 1)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. precedence with a failing final-polynomial (and fold) comparison: one expectation each from the documented order
# ---------------------------------------------------------------------------------------------------------------------
def test_precedence_around_a_final_polynomial_that_fails_in_query_0(layers):
    """final_poly_first: coefficient 0 is off by one, so the final comparison fails in EVERY query, query 0 included.
    Trees 4 and 5 of a query round are FRI layers 0 and 1."""
    L, bad = layers.L, layers.named("final_poly_first").proof
    over = bad.copy()
    over[L.final_poly + 5] = np.uint64(P)
    over_leaf = bad.copy()
    over_leaf[L.leaf(27, 5, 3)] = np.uint64((1 << 64) - 1)
    layers.same_as_oracle([flipped(bad, L.sibling(9, 4, 1)), flipped(bad, L.sibling(1, 5, 6))], [FINAL_POLY, FINAL_POLY])
    layers.same_as_oracle([flipped(bad, L.sibling(0, 4, 1)), flipped(bad, L.sibling(0, 5, 6))], [FRI_MERKLE, FRI_MERKLE])
    layers.same_as_oracle([flipped(bad, L.sibling(0, 1, 3)), flipped(bad, L.sibling(0, 3, 21))], [INITIAL_MERKLE, INITIAL_MERKLE])
    # a word >= p has no oracle verdict (the oracle reduces): the documented order alone puts it first
    assert layers.c.verify(np.stack([over, bad, over_leaf, layers.proof])).tolist() == [MALFORMED, FINAL_POLY, MALFORMED, OK]


def test_precedence_around_a_fold_that_fails_in_every_query(layers):
    """fri_fold0: layer 1 commits to a wrong fold of layer 0, so layer 1's evaluation check fails in every query.  Inside
    a layer the evaluation check precedes the Merkle path; layer 0's path precedes layer 1's evaluation."""
    L, bad = layers.L, layers.named("fri_fold0").proof
    layers.same_as_oracle([flipped(bad, L.sibling(0, 5, 2)), flipped(bad, L.sibling(0, 4, 2)), flipped(bad, L.sibling(3, 4, 2))],
                          [FRI_EVAL, FRI_MERKLE, FRI_EVAL])


def test_precedence_without_fri_layers(flat):
    """The `and` gadget: the batched polynomial is the final polynomial, FINAL_POLY is the only FRI comparison."""
    L, bad = flat.L, flat.named("opening_wire_unread").proof
    over = bad.copy()
    over[L.public_inputs - 1] = np.uint64(P + 1)          # the PoW witness
    flat.same_as_oracle([flipped(bad, L.sibling(5, 2, 1)), flipped(bad, L.sibling(0, 2, 1)), flipped(bad, L.leaf(0, 0, 1))],
                        [FINAL_POLY, INITIAL_MERKLE, INITIAL_MERKLE])
    assert flat.c.verify(np.stack([over, bad])).tolist() == [MALFORMED, FINAL_POLY]


# ---------------------------------------------------------------------------------------------------------------------
# 3. recursion on the device: a forged inner proof has no witness, its honest neighbours are proved
# ---------------------------------------------------------------------------------------------------------------------
def no_witness_between_honest_neighbours(outer, honest, forged):
    for f in forged:
        proofs, st = outer.prove(np.stack([honest, f.proof, honest]), seeds=[7, 7, 7])
        assert st.tolist() == [0, WITNESS_CONFLICT, 0], f.name
        assert (proofs[0] == proofs[2]).all() and proofs[0].any(), f.name


def test_recursive_verifier_refuses_every_forged_inner_proof(flat, layers):
    """The recursive verifier of the `and` gadget, with every fault that applies to its inner circuit."""
    no_witness_between_honest_neighbours(layers.c, flat.proof, flat.forged)
    dg, cap = layers.c.digest()
    proofs, st = layers.c.prove(flat.proof[None, :], seeds=[7])
    assert st.tolist() == [0] and layers.oc.verify(proofs[0], dg, cap)[0] == 0


def test_depth_two_refuses_forged_fri_layers_and_folds(layers):
    outer2 = layers.c.build_recursive_verifier(1)
    forged = [f for f in layers.forged if f.kind in (fp.FRI_LAYER, fp.FRI_FOLD)]
    assert len(forged) == 6
    no_witness_between_honest_neighbours(outer2, layers.proof, forged)
    outer2.close()


def test_aggregator_refuses_one_forged_child(flat):
    """A 2-to-1 aggregation of `and` proofs: a forged child on either side, among honest pairs."""
    agg = flat.c.build_aggregator(2)
    good, f0, f1 = flat.proof, flat.named("final_poly_last_imag").proof, flat.named("opening_zs_next").proof
    pairs = np.stack([np.concatenate(p) for p in ((good, good), (good, f0), (f1, good), (good, good))])
    _proofs, st = agg.prove(pairs, seeds=[1, 2, 3, 4])
    assert st.tolist() == [0, WITNESS_CONFLICT, WITNESS_CONFLICT, 0]
    agg.close()
