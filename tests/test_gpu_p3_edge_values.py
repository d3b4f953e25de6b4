"""GPU: the device plonky3 prover and verifier (P3Prover) on boundary-valued traces (tests/air_cases_edge.py).

The other P3Prover tests prove Fibonacci, `squares`, random recurrences, MiMC and LogUp traces: pseudo-random words, on which
the rare paths of device gl::mul (the asm), of the lazy NTT under ntt_inverse / ntt_lde_bitrev and of the F_p^2 kernels have
probability about 2^-32 per operation.  Here the traces have FREE columns filled from tests/edge_values.py, the other columns
derived in Python integers, so that k_p3_quotient's run_air, k_p3_eval, k_p3_identity, k_p3_reduced, k_p3_fold and the
auxiliary-column kernels compute on 0, 1, p - 1, 2^32 +- 1, ... and on what the transforms make of structured columns.

Yardstick and rule of tests/test_gpu_p3_prover.py: P3Prover.prove returns THE WORDS of the host prover p3_prove_air (whose
arithmetic is reduce128, not the asm), np.array_equal, status for status, and every word is canonical; the host's words on
this data are held to the Python models and to the oracle's verifier circuit by tests/test_p3_edge_values_cpu.py.  The
verifier's verdicts are those of tests/p3_verify_model.py / p3_aux_model.py."""
import numpy as np
import pytest

import air_cases_aux
import air_cases_edge as edge
import edge_values as ev
import p3_verify_cases as pc
import p3_verify_model as M
from conftest import P

pytestmark = pytest.mark.gpu
PU = np.uint64(P)
OK = 0
QUERIES, POW_BITS = 3, 4

# the smallest log_n of test_gpu_p3_prover_forms.py::test_two_pass_transform_at_every_blowup: the first two-pass transform,
# read from kernels_ntt.hip
TWO_PASS_LOG_N = ev.ntt_source_constants()["TWO_PASS_LOG"]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got < PU).all(), (what, "non-canonical word at", np.argwhere(got >= PU)[:5].tolist())
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing words", bad[:5].tolist(), len(bad), "of", got.size)


def _host(gpu, air, trace, q, pow_bits, log_blowup, pv=None, threads=None):
    """The host prover's words; it raises (status 1) for a trace that violates the AIR or has a zero denominator."""
    return gpu.p3_prove_air(air, trace, num_queries=q, pow_bits=pow_bits, log_blowup=log_blowup, public_values=pv,
                            threads=threads)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 1. every EDGE x EDGE pair through device mul, add and sub
# ---------------------------------------------------------------------------------------------------------------------
def test_every_edge_pair_as_a_constant_trace(gpu):
    """free_ops with the constant trace (u, v, u v, u + v, u - v) for every ordered pair (u, v) of EDGE, as ONE batch: one
    proof per pair.  A constant column's LDE is constant, so run_air executes mul, add and sub on exactly (u, v) at every
    point of the quotient coset.  The true quotient is zero: a single wrong device product, sum or difference turns into
    non-zero quotient words or a failed identity (status 1 and a zero row), and either differs from the host's proof.
    log_n 3, 2 queries, no proof of work."""
    log_n, q = 3, 2
    air = edge.free_ops(gpu)
    traces = edge.free_ops_constant_traces(log_n)
    n = len(edge.EDGE) ** 2
    assert traces.shape == (n, 8, 5) and n == 400
    pr = gpu.P3Prover(air, log_n, 1, q, 0)
    got, st = pr.prove(traces)
    assert st.tolist() == [OK] * n, [edge.constant_pairs()[i] for i in np.nonzero(st)[0][:5]]
    s = M.Shape(pr.config)
    for i, pair in enumerate(edge.constant_pairs()):
        _same(got[i], _host(gpu, air, traces[i], q, 0, 1, threads=1), ("pair", [hex(v) for v in pair]))
    # zero by construction: the quotient chunk's openings, every FRI sibling value and the final polynomial
    assert not got[:, s.o_chunks:s.o_chunks + 4 * s.Q].any() and not got[:, s.o_final_poly:s.o_final_poly + 2].any()
    assert not any(got[:, s.step(j, r):s.step(j, r) + 2].any() for j in range(q) for r in range(s.k))
    assert pr.verify(got).tolist() == [OK] * n
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fills in the free columns of the three base-field families
# ---------------------------------------------------------------------------------------------------------------------
# every fill pair at every height: the host's 22 proofs at 2^11 rows take 1 to 2 s, everything else less
LOG_NS = (3, 6, TWO_PASS_LOG_N)
BASE_CASES = [(fam, log_n, lb) for fam, (_a, _t, _d, lbs) in edge.FAMILIES.items() for log_n in LOG_NS for lb in lbs]


@pytest.mark.parametrize("family,log_n,log_blowup", BASE_CASES)
def test_base_field_families_on_boundary_fills(gpu, family, log_n, log_blowup):
    """Every fill pair as a lone proof (the first and the last at 2^11 rows) and all of them as one group: the host's words,
    and the device verifier accepts them."""
    make_air, _make_trace, degree, _lbs = edge.FAMILIES[family]
    air = make_air(gpu)
    named = edge.traces(family, log_n)
    traces = np.stack([t for _name, t in named])
    pr = gpu.P3Prover(air, log_n, log_blowup, QUERIES, POW_BITS)
    assert 1 << pr.config.log_quotient_degree == {2: 1, 3: 2, 5: 4}[degree]
    want = [_host(gpu, air, t, QUERIES, POW_BITS, log_blowup) for t in traces]
    got, st = pr.prove(traces)
    assert st.tolist() == [OK] * len(named)
    for i, (name, _t) in enumerate(named):
        _same(got[i], want[i], (family, log_n, log_blowup, name, "in the group"))
    lone = range(len(named)) if log_n <= 6 else (0, len(named) - 1)
    for i in lone:
        one, st1 = pr.prove(traces[i])
        assert st1.tolist() == [OK]
        _same(one[0], want[i], (family, log_n, log_blowup, named[i][0], "alone"))
    assert pr.verify(got).tolist() == [OK] * len(named)
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. F_p^2: the auxiliary-column kernels, k_p3_quotient<ExtF>, the preprocessed and periodic loads
# ---------------------------------------------------------------------------------------------------------------------
def test_the_third_height_is_the_first_two_pass_transform():
    assert TWO_PASS_LOG_N == 11 and LOG_NS == (3, 6, 11), "a threshold moved: the 2^11-row cases no longer sit on it"


def test_the_big_height_takes_a_second_totals_tile():
    block, tile = air_cases_aux.scan_constants()
    assert (1 << edge.EXT_LOG_BIG) == 2 * block * tile and edge.EXT_LOG_BIG == air_cases_aux.BIG_SHAPES[1][3]


@pytest.mark.parametrize("log_n", [edge.EXT_LOG_SMALL, edge.EXT_LOG_BIG])
@pytest.mark.parametrize("kind", ["edge_range", "edge_pvper"])
def test_logup_on_boundary_words(gpu, kind, log_n):
    """The condition, from the host alone: it proves the trace (status 0), so no denominator is zero."""
    big = log_n == edge.EXT_LOG_BIG
    q, pow_bits = (2, 0) if big else (QUERIES, POW_BITS)
    air, trace, pv = edge.ext_case(gpu, kind, log_n)
    want = _host(gpu, air, trace, q, pow_bits, 1, pv, threads=16 if big else 1)
    pr = gpu.P3Prover(air, log_n, 1, q, pow_bits)
    got, st = pr.prove(trace, public_values=pv)
    assert st.tolist() == [OK]
    _same(got[0], want, (kind, log_n))
    if not big:                      # in a group too, three instances
        made = [edge.ext_case(gpu, kind, log_n, seed) for seed in (0, 1, 2)]
        rows, st = pr.prove(np.stack([m[1] for m in made]), public_values=None if pv is None else np.stack([m[2] for m in made]))
        assert st.tolist() == [OK] * 3
        for (a, t, v), row in zip(made, rows):
            _same(row, _host(gpu, a, t, q, pow_bits, 1, v, threads=1), (kind, log_n, "group"))
    assert pr.verify(got).tolist() == [OK]
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the verifier on a proof full of zeros
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zero_proof(gpu, oracle):
    """free_ops on the constant trace of (p - 1, 2^32 - 1) at 2^2 rows, 2 queries, from the DEVICE prover: zero chunks, zero
    FRI layers, a zero final polynomial."""
    air = edge.free_ops(gpu)
    pair = (P - 1, (1 << 32) - 1)
    trace = edge.free_ops_constant_traces(2)[edge.constant_pairs().index(pair)]
    pr = gpu.P3Prover(air, 2, 1, 2, 0)
    got, st = pr.prove(trace)
    assert st.tolist() == [OK]
    _same(got[0], _host(gpu, air, trace, 2, 0, 1, threads=1), "the zero proof")
    s = M.Shape(pr.config)
    assert np.count_nonzero(got[0] == 0) >= 4 * s.Q + 2 + 2 * 2 * s.k
    assert M.verify(oracle, air, pr.config, got[0]) == M.OK
    yield air, pr, got[0]
    pr.close()


def test_every_flip_of_a_proof_full_of_zeros(gpu, oracle, zero_proof):
    air, pr, words = zero_proof
    flips = pc.all_flips(words)
    assert len(flips) >= words.size - 16                  # all but the words that are p - 1 (the flip would leave the field)
    batch = np.stack([words] + [w for _pos, w in flips])
    want = [M.verify(oracle, air, pr.config, w) for w in batch]
    got = pr.verify(batch)
    assert got.tolist() == want, [(i - 1, int(g), w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    assert want[0] == M.OK and {M.INPUT_MERKLE, M.FRI_MERKLE, M.FINAL_POLY} <= set(want[1:])
    assert pr.verify(batch[::-1].copy()).tolist() == want[::-1]


def test_words_at_or_above_p_in_a_proof_full_of_zeros(gpu, oracle, zero_proof):
    air, pr, words = zero_proof
    batch = np.stack([pc.with_word(words, pos, word) for pos in range(words.size) for word in (P, (1 << 64) - 1)])
    want = [M.verify(oracle, air, pr.config, w) for w in batch]
    assert set(want) == {M.MALFORMED}
    assert pr.verify(batch).tolist() == want
