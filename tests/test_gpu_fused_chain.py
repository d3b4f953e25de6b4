"""GPU: the fused launches of a proof's serial chain -- the multi-segment transcript launch with its copies and closing
actions, the openings as one job-table grid, the one-grid PoW search -- each against the oracle, or against the
one-segment / one-job form of the same kernel."""
import numpy as np
import pytest

import reference_vectors as rv
from conftest import P, splitmix_field

pytestmark = pytest.mark.gpu

RATE_LENGTHS = [0, 1, 7, 8, 9, 64, 516]       # around the sponge rate (8), one wave's load (64) and beyond it


def test_transcript_scripts_of_1_to_9_segments_vs_oracle(gpu, oracle):
    """Four segments go to a launch and a launch ends where challenges are drawn: scripts of 1 to 9 segments with
    challenges after some segments only cover every packing (1..4 segments per launch, with and without a draw)."""
    rng = np.random.default_rng(2024)
    for n_seg in range(1, 10):
        for trial in range(3):
            segs = []
            for k in range(n_seg):
                n_obs = RATE_LENGTHS[(3 * k + 5 * trial + n_seg) % len(RATE_LENGTHS)]
                n_ch = int(rng.choice([0, 0, 0, 1, 2, 9])) if k + 1 < n_seg else 3       # always ends on a draw
                segs.append((splitmix_field(n_obs, seed=1000 * n_seg + 10 * trial + k + 1), n_ch))
            got, want = gpu.transcript(segs), oracle.transcript(segs)
            assert got.shape == want.shape and (got == want).all(), (n_seg, trial, [(len(w), c) for w, c in segs])
            assert (got < np.uint64(P)).all()
    # no draw until the very end: 9 segments = 4 + 4 + 1
    segs = [(splitmix_field(RATE_LENGTHS[k % 7], seed=50 + k), 0) for k in range(8)] + [(splitmix_field(9, seed=60), 5)]
    assert (gpu.transcript(segs) == oracle.transcript(segs)).all()


def test_transcript_does_not_depend_on_how_a_script_is_cut(gpu, oracle):
    words = splitmix_field(516 + 64 + 9, seed=77)
    whole = gpu.transcript([(words, 11)])
    assert (whole == oracle.transcript([(words, 11)])).all()
    for cuts in ([8], [1, 9], [7, 64, 516], [0, 0, 1, 8, 72, 73, 580], [64, 128, 192, 256, 320, 384, 448, 512]):
        edges = [0] + cuts + [words.size]
        segs = [(words[a:b], 0) for a, b in zip(edges[:-1], edges[1:])]
        segs[-1] = (segs[-1][0], 11)
        assert (gpu.transcript(segs) == whole).all(), cuts


@pytest.mark.parametrize("log_n", [10, 16])
def test_openings_1_2_85_135_polynomials_vs_oracle(gpu, oracle, log_n):
    zeta = splitmix_field(2, seed=171)
    g = pow(1753635133440165772, 1 << (32 - log_n), P)
    for n_polys in (1, 2, 85, 135):
        coeffs = splitmix_field(n_polys << log_n, seed=170 + n_polys).reshape(n_polys, 1 << log_n)
        for scale in (1, g):
            got, want = gpu.eval_polys(coeffs, zeta, scale), oracle.eval_polys(coeffs, zeta, scale)
            assert got.shape == want.shape and (got == want).all(), (log_n, n_polys, scale)


def test_openings_chunked_path_vs_oracle(gpu, oracle):
    log_n, n_polys = 17, 3
    coeffs = splitmix_field(n_polys << log_n, seed=190).reshape(n_polys, 1 << log_n)
    zeta = splitmix_field(2, seed=191)
    g = pow(1753635133440165772, 1 << (32 - log_n), P)
    for scale in (1, g):
        assert (gpu.eval_polys(coeffs, zeta, scale) == oracle.eval_polys(coeffs, zeta, scale)).all(), scale


@pytest.mark.parametrize("pow_bits", [0, 8, 16, 20])
def test_pow_search_finds_the_smallest_witness_twice(gpu, oracle, pow_bits):
    """The oracle's proof holds the smallest witness (upstream searches upwards from 0); the query indices and openings
    behind it depend on it, so the whole proof is compared."""
    log_n, rate_bits, cap_h, arity, queries = 8, 2, 2, [3, 2], 4
    coeffs = splitmix_field(2 << log_n, seed=300 + pow_bits).reshape(2, 1 << log_n)
    seed = splitmix_field(5, seed=301)
    want = oracle.fri_prove(coeffs, rate_bits, cap_h, arity, pow_bits, queries, seed)
    for _ in range(2):
        got, st = gpu.fri_prove(coeffs, rate_bits, cap_h, arity, pow_bits, queries, seed)
        assert st == 0
        assert got.shape == want.shape and (got == want).all(), np.nonzero(got != want)[0][:8]


def test_fib64_proof_equals_the_oracles(gpu, fib_circuit, fib_oracle, fib_inputs):
    """Every word: the caps (stored by the transcript launches), openings, final polynomial, PoW witness, queries."""
    proofs, st = fib_circuit.prove(fib_inputs[None, :], seeds=[5])
    want, sto, _t, msg = fib_oracle.prove(fib_inputs, seed=5)
    assert st.tolist() == [0] and sto == 0, (st.tolist(), sto, msg)
    diff = np.nonzero(proofs[0] != want)[0]
    assert diff.size == 0, f"first differing words {diff[:8]} of {want.size}"


def test_gadget_proof_with_public_inputs_equals_the_oracles(gpu, oracle):
    """The preamble holds this proof's public-inputs hash, and it is observed in the same launch as the wires cap."""
    c = gpu.Circuit.build_gadget(13, 0)
    assert int(c.info.num_public_inputs) == 2
    oc = oracle.load_circuit(c.to_blob())
    inp = np.array([rv.UNINTERLEAVE_X], dtype=np.uint64)
    proofs, st = c.prove(inp[None, :], seeds=[9])
    want, sto, _t, msg = oc.prove(inp, seed=9)
    assert st.tolist() == [0] and sto == 0, (st.tolist(), sto, msg)
    assert (proofs[0] == want).all(), np.nonzero(proofs[0] != want)[0][:8]
    assert [int(v) for v in c.public_inputs(proofs[0])] == [rv.UNINTERLEAVE_EVENS_EXPECTED, rv.UNINTERLEAVE_ODDS_EXPECTED]
    c.close()
