"""GPU: p25_verify_batch / p25_verify_batch_dev against the oracle's verifier.

The yardstick is always `oc.verify(proof, digest, cap)[0]` (oracle/ref_prover.cpp `ref_verify`, one code per failing
check), mapped to the library's verdicts by `0 if code == 0 else code + 10`.  Shapes are the smallest that still reach
the code: the gadget circuits (2^2 .. 2^5 rows, no FRI layer), the recursive verifier over the `and` gadget (2^11 rows,
FRI layers, the recursion gate set) and one fib-64 proof.

Editing a finished proof cannot produce P25_REJECT_FINAL_POLY, nor reach the check of the openings against the
commitments: any such change moves the PoW response and the query indices, so the proof is rejected with 20, 21 or 23
first.  Those comparisons are reached by the forged proofs of tests/test_gpu_forged_proofs.py."""
import numpy as np
import pytest

import gadget_cases
import reference_vectors as rv
from conftest import P
from device_buffers import Banded, Banded32, SENTINEL32, strided_rows
from verify_cases import (CAP_WORDS, FRI_EVAL, FRI_MERKLE, INITIAL_MERKLE, INVALID_ARG, MALFORMED, OK, POW, VANISHING, Layout,
                          expected, flipped, reference_gates_inputs)

pytestmark = pytest.mark.gpu

class Case:
    def __init__(self, c, oc, proof):
        self.c, self.oc, self.proof = c, oc, proof
        self.dg, self.cap = c.digest()
        self.L = Layout(c)
        self.pw = int(c.info.proof_words)

    def parity(self, batch):
        """One verify call over `batch`; per proof the oracle's verdict.  Returns (gpu statuses, oracle statuses)."""
        got = self.c.verify(batch)
        want = np.array([expected(self.oc, p, self.dg, self.cap) for p in batch], dtype=np.int32)
        return got, want


def proved(gpu, oracle, c, inputs, seed=3):
    proofs, st = c.prove(np.asarray(inputs, dtype=np.uint64)[None, :], seeds=[seed])
    assert st.tolist() == [0]
    return Case(c, oracle.load_circuit(c.to_blob()), proofs[0])


@pytest.fixture(scope="module")
def and_case(gpu, oracle):
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    return proved(gpu, oracle, gpu.Circuit.build_gadget(0, 0), [x, y, (x & y) % P], seed=5)


@pytest.fixture(scope="module")
def rec_case(gpu, oracle, and_case):
    """The recursive verifier over the `and` gadget: 2^11 rows, FRI layers, the recursion gate set."""
    outer = and_case.c.build_recursive_verifier(1)
    case = proved(gpu, oracle, outer, and_case.proof, seed=1)
    assert int(outer.info.degree_bits) == 11 and case.L.n_layers >= 1
    return case


@pytest.fixture(scope="module")
def fib_case(gpu, fib_circuit, fib_oracle, fib_inputs):
    proofs, st = fib_circuit.prove(fib_inputs[None, :], seeds=[11])
    assert st.tolist() == [0]
    return Case(fib_circuit, fib_oracle, proofs[0])


# ---------------------------------------------------------------------------------------------------------------------
# 1. accepts what the prover makes
# ---------------------------------------------------------------------------------------------------------------------
def accepts(case):
    got = case.c.verify(np.stack([case.proof, case.proof]))
    assert got.dtype == np.int32 and got.tolist() == [OK, OK]
    assert case.oc.verify(case.proof, case.dg, case.cap)[0] == 0


def test_accepts_every_gadget_proof(gpu, oracle):
    for name, kind, param, inputs in gadget_cases.cases(oracle):
        case = proved(gpu, oracle, gpu.Circuit.build_gadget(kind, param), inputs)
        assert int(case.c.info.degree_bits) <= 7 and case.L.n_layers == 0, name
        accepts(case)
        case.c.close()


def test_accepts_public_inputs_and_the_reference_gates(gpu, oracle):
    """Gadgets 11 (public inputs), 12, 13 and 14: U32Interleave, UninterleaveToU32, U32Arithmetic and Poseidon2 gates, two
    selector groups."""
    xs = [(0x9E3779B97F4A7C15 * (i + 1)) % P for i in range(3)]
    for kind, param, inputs in ((11, 3, xs), (12, 0, [rv.INTERLEAVE_X]), (13, 0, [rv.UNINTERLEAVE_X]),
                                (14, 0, reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF))):
        case = proved(gpu, oracle, gpu.Circuit.build_gadget(kind, param), inputs)
        accepts(case)
        if kind == 14:
            assert int(case.c.info.num_selectors) == 2
        case.c.close()


def test_accepts_the_recursive_verifier_proof(rec_case):
    accepts(rec_case)


def test_accepts_a_fib64_proof(fib_case):
    assert fib_case.pw == 19861 and fib_case.L.n_layers == 3
    accepts(fib_case)


# ---------------------------------------------------------------------------------------------------------------------
# 2., 3. single-word tamper parity
# ---------------------------------------------------------------------------------------------------------------------
def test_single_word_tamper_parity_and_gadget(and_case):
    """Bit 0 of one word flipped per proof: every third word ahead of the first query round, every 97th behind it."""
    L = and_case.L
    assert and_case.pw == 9193
    words = list(range(0, L.queries, 3)) + list(range(L.queries, and_case.pw, 97))
    got, want = and_case.parity(np.stack([flipped(and_case.proof, w) for w in words]))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(words[i], int(got[i]), int(want[i])) for i in bad[:8]]
    assert set(want.tolist()) == {VANISHING, POW, INITIAL_MERKLE}
    # two opening words the vanishing identity does not see: the oracle answers with the PoW there, and so must the GPU
    got, want = and_case.parity(np.stack([flipped(and_case.proof, w) for w in (626, 627)]))
    assert got.tolist() == want.tolist() == [POW, POW]


def test_single_word_tamper_parity_with_fri_layers(rec_case):
    """The same over the recursive verifier's proof at stride 41: all of 20, 21, 23, 24 and 25 occur."""
    assert rec_case.pw == 15189
    words = list(range(0, rec_case.pw, 41))
    assert len(words) == 371
    got, want = rec_case.parity(np.stack([flipped(rec_case.proof, w) for w in words]))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(words[i], int(got[i]), int(want[i])) for i in bad[:8]]
    assert set(want.tolist()) == {VANISHING, POW, INITIAL_MERKLE, FRI_EVAL, FRI_MERKLE}


# ---------------------------------------------------------------------------------------------------------------------
# 4. fib-64: one flipped word per layout section
# ---------------------------------------------------------------------------------------------------------------------
def test_fib64_one_flip_per_layout_section(fib_case):
    L, q = fib_case.L, 13
    words = {"wires_cap": L.wires_cap + 5, "zs_cap": L.zs_cap + 17, "quotient_cap": L.quotient_cap + 63,
             "constants": L.constants + 1, "sigmas": L.sigmas + 7, "wires": L.wires + 100, "zs": L.zs + 1,
             "zs_next": L.zs_next + 2, "pps": L.pps + 9, "quotient": L.quotient + 30, "fri_cap": L.fri_caps + CAP_WORDS + 3,
             "final_poly": L.final_poly + 3, "pow_witness": L.pow_witness}
    for t in range(4):
        words[f"leaf{t}"] = L.leaf(q, t, 2)
        words[f"sibling{t}"] = L.sibling(q, t, 9)
    for l in range(L.n_layers):
        words[f"evals{l}"] = L.leaf(q, 4 + l, 5)
        words[f"fri_sibling{l}"] = L.sibling(q, 4 + l, 6)
    names = sorted(words)
    got, want = fib_case.parity(np.stack([flipped(fib_case.proof, words[n]) for n in names]))
    assert got.tolist() == want.tolist(), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
    assert (want != 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. precedence: the first failure of the sequential verifier, not the last writer
# ---------------------------------------------------------------------------------------------------------------------
def test_precedence_between_queries(rec_case):
    L = rec_case.L
    fri_then_leaf = flipped(rec_case.proof, L.sibling(5, 4, 1), L.leaf(9, 1, 3))
    leaf_then_fri = flipped(rec_case.proof, L.leaf(5, 1, 3), L.sibling(9, 4, 1))
    got, want = rec_case.parity(np.stack([fri_then_leaf, leaf_then_fri]))
    assert want.tolist() == [FRI_MERKLE, INITIAL_MERKLE]
    assert got.tolist() == want.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 6. wrong verifier data
# ---------------------------------------------------------------------------------------------------------------------
def test_wrong_verifier_data(gpu, and_case):
    c, oc, proof = and_case.c, and_case.oc, and_case.proof
    batch = np.stack([proof, proof])
    assert c.verify(batch, and_case.dg, and_case.cap).tolist() == [OK, OK]
    dg = and_case.dg.copy()
    dg[2] ^= np.uint64(1)
    assert c.verify(batch, dg, and_case.cap).tolist() == [VANISHING] * 2 == [expected(oc, proof, dg, and_case.cap)] * 2
    cap = and_case.cap.copy()
    cap[:, 0] ^= np.uint64(1)           # every entry of the cap
    assert c.verify(batch, and_case.dg, cap).tolist() == [INITIAL_MERKLE] * 2 == [expected(oc, proof, and_case.dg, cap)] * 2
    for kw in ({"digest": and_case.dg}, {"cs_cap": and_case.cap}):
        with pytest.raises(gpu.P25Error) as e:
            c.verify(batch, **kw)
        assert e.value.status == INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 7. malformed: a word >= p is not its residue
# ---------------------------------------------------------------------------------------------------------------------
def test_malformed_words_are_rejected(gpu, oracle):
    xs = [(0x9E3779B97F4A7C15 * (i + 1)) % P for i in range(3)]
    case = proved(gpu, oracle, gpu.Circuit.build_gadget(11, 3), xs)
    L = case.L
    assert int(case.c.info.num_public_inputs) == 5
    positions = {"cap": L.zs_cap + 5, "opening": L.wires + 3, "leaf": L.leaf(0, 0, 2), "final_poly": L.final_poly + 1,
                 "public_input": L.public_inputs + 1}
    batch, bad_at = [case.proof], []
    for name in sorted(positions):
        for word in (P, (1 << 64) - 1, P + 5):
            q = case.proof.copy()
            q[positions[name]] = np.uint64(word)
            bad_at.append(len(batch))
            batch += [q, case.proof]
    got = case.c.verify(np.stack(batch))
    want = np.zeros(len(batch), dtype=np.int32)
    want[bad_at] = MALFORMED
    assert got.tolist() == want.tolist()
    case.c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. batch mechanics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def and_pool(and_case):
    """The valid proof and tampered versions of it with the oracle's verdicts: what batches are drawn from."""
    L = and_case.L
    pool = [and_case.proof] + [flipped(and_case.proof, w) for w in (L.wires + 8, L.pow_witness, L.leaf(0, 1, 1),
                                                                    L.sibling(27, 3, 2), L.zs_cap + 1)]
    codes = np.array([expected(and_case.oc, p, and_case.dg, and_case.cap) for p in pool], dtype=np.int32)
    assert codes[0] == OK and set(codes[1:].tolist()) == {VANISHING, POW, INITIAL_MERKLE}
    return np.stack(pool), codes


def strided_batch(pool, pick, stride):
    rows = np.full((len(pick), stride), (1 << 64) - 1, dtype=np.uint64)    # poisoned padding
    rows[:, :pool.shape[1]] = pool[pick]
    return rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_strides_and_composition(and_case, and_pool, n):
    pool, codes = and_pool
    pw, stride = and_case.pw, and_case.pw + 3
    pick = np.random.default_rng(1000 + n).integers(0, len(pool), size=n)
    rows = strided_batch(pool, pick, stride)
    assert and_case.c.verify(rows, proof_stride=stride).tolist() == codes[pick].tolist()
    # device form: the same statuses, proofs and padding unchanged, nothing written around either buffer
    d_proofs, d_status = Banded(n * stride), Banded32(n)
    d_proofs.set(rows)
    and_case.c.verify_dev(d_proofs.ptr, n, stride, d_status.ptr)
    and_case.c.sync()
    assert d_status.get().tolist() == codes[pick].tolist()
    d_status.assert_bands_intact()
    d_proofs.assert_unchanged()
    _data, pad = strided_rows(n, pw, stride)
    assert (d_proofs.get()[pad] == np.uint64((1 << 64) - 1)).all()


def test_empty_batch_is_accepted(and_case):
    assert and_case.c.verify(np.zeros((0, and_case.pw), dtype=np.uint64)).size == 0
    d_status = Banded32(4)
    and_case.c.verify_dev(None, 0, and_case.pw, d_status.ptr)
    and_case.c.sync()
    d_status.assert_unchanged()


def test_stride_below_the_proof_is_refused(gpu, and_case):
    with pytest.raises(gpu.P25Error) as e:
        and_case.c.verify(np.zeros((2, and_case.pw - 1), dtype=np.uint64))
    assert e.value.status == INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 9. device-resident form
# ---------------------------------------------------------------------------------------------------------------------
def test_prove_dev_then_verify_dev_without_host_synchronisation(gpu, and_case):
    import torch
    c, n, pw = and_case.c, 20, and_case.pw
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    xy = rng.integers(0, P, size=(n, 2), dtype=np.uint64)
    inputs = np.concatenate([xy, (xy[:, :1] & xy[:, 1:]) % np.uint64(P)], axis=1)
    d_in = torch.from_numpy(inputs.view(np.int64)).to(dev)
    d_seeds = torch.arange(n, dtype=torch.int64, device=dev)
    d_proofs, d_prove_status, d_status = Banded(n * pw), Banded32(n), Banded32(n)
    torch.cuda.synchronize()
    c.prove_dev(d_in.data_ptr(), n, d_seeds.data_ptr(), d_proofs.ptr, pw, d_prove_status.ptr)
    c.verify_dev(d_proofs.ptr, n, pw, d_status.ptr)
    c.sync()
    assert d_prove_status.get().tolist() == [0] * n
    assert d_status.get().tolist() == [OK] * n
    d_status.assert_bands_intact()
    # the proofs the verifier accepted are the oracle's kind of valid
    first = d_proofs.get()[:pw]
    assert and_case.oc.verify(first, and_case.dg, and_case.cap)[0] == 0


def test_joined_stream_sees_the_final_statuses(and_case, and_pool):
    import torch
    pool, codes = and_pool
    n = 33
    pick = np.random.default_rng(77).integers(0, len(pool), size=n)
    d_proofs, d_status = Banded(n * and_case.pw), Banded32(n)
    d_proofs.set(pool[pick])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    and_case.c.verify_dev(d_proofs.ptr, n, and_case.pw, d_status.ptr)
    and_case.c.stream_join(side.cuda_stream)
    with torch.cuda.stream(side):
        seen = d_status._t[d_status.before:d_status.before + n].clone()
    side.synchronize()
    got = seen.cpu().numpy().view(np.uint32)
    assert (got != SENTINEL32).all() and got.tolist() == codes[pick].tolist()
    and_case.c.sync()
