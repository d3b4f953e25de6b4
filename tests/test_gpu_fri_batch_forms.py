"""GPU: the forms the FRI leaf hashes and the PoW search take when several proofs are in flight -- cooperative leaf
hashing for layers of at most COOP_FRI_LEAVES_BATCH leaves, the per-lane kernel at wave priority 1 in 64-lane workgroups
above it, the PoW search at priority 1 -- against the lone-proof forms of the same proofs and against the oracle.
A call that proves two or more rows has as many proofs in flight and takes the batch forms; a call with one row takes
the lone-proof forms."""
import os
import re

import numpy as np
import pytest

import circuit_bytes_reader as cr
from conftest import ROOT

pytestmark = pytest.mark.gpu

COOP_FRI_LEAVES_BATCH = 2048      # kernels_fri.hip; test_threshold_constant_is_the_one_the_tests_assume reads it back


def fri_layer_leaves(c):
    """Leaves of each FRI layer's tree, from the circuit's own serialised FRI parameters (the head of its CircuitData
    bytes) and circuit.info.degree_bits."""
    r = cr.Reader(c.to_bytes())
    for _ in range(6):
        r.usize()
    r.boolean(), r.boolean()
    cfg = r.fri_config()
    r.fri_config()
    arity_bits = r.vec_usize()
    assert r.usize() == int(c.info.degree_bits)
    bits, leaves = int(c.info.degree_bits) + cfg["rate_bits"], []
    for a in arity_bits:
        leaves.append(1 << (bits - a))
        bits -= a
    return leaves, arity_bits, cfg


def test_threshold_constant_is_the_one_the_tests_assume():
    src = open(os.path.join(ROOT, "plonky2.5_amd", "csrc", "kernels_fri.hip")).read()
    m = re.search(r"COOP_FRI_LEAVES_BATCH\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == COOP_FRI_LEAVES_BATCH


def test_fib64_proofs_in_flight_together_equal_the_same_proofs_alone(gpu, fib_circuit, fib_inputs):
    """Three rows, three seeds, one call: layer 2^15 per-lane at priority 1, layers 2^11 and 2^7 cooperative, PoW at
    priority 1.  Each proof equals, byte for byte, the proof of the same row and seed proved alone (the forms that
    test_fib64_proof_equals_the_oracles pins to the oracle)."""
    leaves, _ab, _cfg = fri_layer_leaves(fib_circuit)
    assert leaves == [1 << 15, 1 << 11, 1 << 7]
    rows = np.stack([fib_inputs] + [gpu.p3_prove_fibonacci(6, 100, 16, pow_start=v << 24)[0] for v in (1, 2)])
    seeds = [5, 6, 7]
    together, st = fib_circuit.prove(rows, seeds=seeds)
    assert st.tolist() == [0, 0, 0]
    for i, seed in enumerate(seeds):
        alone, st1 = fib_circuit.prove(rows[i][None, :], seeds=[seed])
        assert st1.tolist() == [0]
        diff = np.nonzero(together[i] != alone[0])[0]
        assert diff.size == 0, f"proof {i}: first differing words {diff[:8]} of {alone[0].size}"
    assert (together[0] != together[1]).any() and (together[1] != together[2]).any()


SMALL_SEEDS = [21, 22, 23, 24]


@pytest.fixture(scope="module")
def small_case(gpu, oracle):
    """The verifier circuit of 2^12 rows (the shape of test_gpu_p3_shapes' (4, 10, 8)): its first FRI layer has exactly
    COOP_FRI_LEAVES_BATCH leaves.  Two input rows alternating under four seeds, and the oracle's proof of each, computed
    once for the tests below."""
    inp, cfg = gpu.p3_prove_fibonacci(4, 10, 8)
    other, _ = gpu.p3_prove_fibonacci(4, 10, 8, pow_start=1 << 20)
    c = gpu.Circuit.build_p3_verifier(cfg)
    rows = np.stack([inp, other, inp, other])
    return c, rows, oracle_proofs(oracle.load_circuit(c.to_blob()), rows, SMALL_SEEDS)


def oracle_proofs(oc, rows, seeds):
    want = []
    for row, seed in zip(rows, seeds):
        proof, sto, _tm, msg = oc.prove(row, seed=seed)
        assert sto == 0, msg
        want.append(proof)
    return want


def prove_together(c, rows, seeds, want):
    proofs, st = c.prove(rows, seeds=seeds)
    assert st.tolist() == [0] * len(seeds)
    for i, seed in enumerate(seeds):
        diff = np.nonzero(proofs[i] != want[i])[0]
        assert diff.size == 0, (i, seed, diff[:8])
    return proofs


def test_first_layer_of_exactly_the_threshold_is_cooperative(gpu, small_case):
    c, rows, want = small_case
    assert int(c.info.degree_bits) == 12
    leaves, _ab, _cfg = fri_layer_leaves(c)
    assert leaves[0] == COOP_FRI_LEAVES_BATCH and all(n <= COOP_FRI_LEAVES_BATCH for n in leaves)
    prove_together(c, rows[:2], SMALL_SEEDS[:2], want[:2])


def test_first_layer_of_twice_the_threshold_is_per_lane(gpu, oracle):
    """2^13 rows (test_gpu_p3_shapes' (6, 12, 8)): the first layer, 2 x COOP_FRI_LEAVES_BATCH leaves, takes the per-lane
    kernel in 64-lane workgroups at priority 1, the layers under it the cooperative one."""
    inp, cfg = gpu.p3_prove_fibonacci(6, 12, 8)
    other, _ = gpu.p3_prove_fibonacci(6, 12, 8, pow_start=1 << 20)
    c = gpu.Circuit.build_p3_verifier(cfg)
    assert int(c.info.degree_bits) == 13
    leaves, _ab, _cfg = fri_layer_leaves(c)
    assert leaves[0] == 2 * COOP_FRI_LEAVES_BATCH and all(n <= COOP_FRI_LEAVES_BATCH for n in leaves[1:])
    rows = np.stack([inp, other])
    prove_together(c, rows, [3, 4], oracle_proofs(oracle.load_circuit(c.to_blob()), rows, [3, 4]))
    c.close()


def test_gadget_circuit_in_flight_together_equals_the_oracle(gpu, oracle):
    """The largest gadget circuit (Poseidon over a 135-word leaf and a Merkle step, 2^5 rows).  The gadget circuits stop at
    2^5 rows, which is the final polynomial's size, so they have NO FRI layer: what this covers is the batch chain with
    nothing between the openings and the priority-1 PoW search.  The circuit builders fix the FRI arity at 16 (32-word
    leaves), so no whole proof of any size has a layer of leaves of at most four words (the unhashed ones, which stay on
    the per-lane kernel in either form); test_gpu_stages' test_fri_prove_vs_oracle reaches those through the stage entry
    point, on the lone-proof forms."""
    from gadget_cases import cases
    _n, kind, param, vals = {k[0]: k for k in cases(oracle)}["poseidon_merkle135_1"]
    c = gpu.Circuit.build_gadget(kind, param)
    assert 2 <= int(c.info.degree_bits) <= 7
    leaves, arity_bits, _cfg = fri_layer_leaves(c)
    assert all(n <= COOP_FRI_LEAVES_BATCH for n in leaves) and all(2 << a > 4 for a in arity_bits)
    rows, seeds = np.stack([np.array(vals, dtype=np.uint64)] * 3), [11, 12, 13]
    prove_together(c, rows, seeds, oracle_proofs(oracle.load_circuit(c.to_blob()), rows, seeds))
    c.close()


def test_pow_search_at_priority_one_finds_the_smallest_witness(gpu, small_case):
    """The oracle's proof holds the smallest witness (upstream searches upwards from 0), and the query indices and
    openings behind it depend on it, so whole proofs are compared: four proofs in one call, each seed a different
    transcript and so a different search.  The circuit builders use the standard recursion configuration
    (proof_of_work_bits = 16) and give no access to another one, so proof_of_work_bits = 0 is not covered here;
    test_pow_search_finds_the_smallest_witness_twice covers it for the priority-0 instance."""
    c, rows, want = small_case
    _leaves, _ab, cfg = fri_layer_leaves(c)
    assert cfg["proof_of_work_bits"] == 16
    proofs = prove_together(c, rows, SMALL_SEEDS, want)
    assert len({p.tobytes() for p in proofs}) == len(SMALL_SEEDS)
