"""GPU: the device plonky3 prover (P3Prover) where its launch forms change, against the host prover.

Yardstick and rule of tests/test_gpu_p3_prover.py: for the same arguments P3Prover.prove returns THE WORDS of p3_prove_air,
np.array_equal, no tolerance, status for status.  The shapes here are the smallest that reach code the other file's
shapes leave unexecuted; each states the condition it crosses and asserts it from the thresholds in p3_kernels.h
(P3_TREE_COOP_MAX, P3_TREE_TOP_NODES, P3_TAIL_LOG, P3_MAX_LIVE), read from the header: a threshold that moves takes the
shapes with it, and a shape that can no longer cross it fails its precondition instead of passing.

  1. k_p3_tree_level (one lane per node), alone and under blockIdx.y > 0, with the equality case on the cooperative side;
     the second trip of the `+= 64` loops of k_p3_gather: Merkle paths (4 L > 64), FRI paths (4 (L - 1) > 64), trace
     columns (W > 64, also 18 permutations per leaf in k_p3_leaf_cols and 2 W + 2 Q > 128 blocks of k_p3_eval);
     FRI rounds 0 .. 7 as separate launches in front of k_p3_fri_tail
  2. the LDE at log_blowup 2, 3, 4 (4 = two ntt_lde_bitrev calls into the halves of the output) with the two-pass
     transform (log_n >= 11) and 2, 4, 8 quotient chunks; the smallest transforms at every blowup
  3. k_p3_pow_search: many trips per lane (18 bits), and the last candidate below p as the only one
  4. (a short last group, 41 proofs in groups of 8: tests/test_gpu_p3_prover.py::test_grouping_changes_no_word)
  5. the register program (P3AirDevice::compile, run_air in k_p3_quotient and k_p3_identity) on generated DAGs with
     sharing: slot release and reuse, a node read by several constraints, a root read again later, x op x; the host
     evaluates the DAG by AirProgram::fold, not by the register program.  One of them through the oracle's verifier
     circuit, a check that does not pass through the host prover
  6. P3_MAX_LIVE: the largest accepted chain, a value in every slot index; a long program through a handful of slots
  7. verdicts cell by cell (k_p3_identity, the zeros of k_p3_gather for a failed proof next to untouched neighbours), and
     constant traces: a zero quotient, all-zero FRI layers, a zero final polynomial"""
import os
import re

import numpy as np
import pytest

import air_cases
from conftest import P, ROOT
from test_gpu_p3_prover import POW_STARTS, _sextic, _sextic_trace

pytestmark = pytest.mark.gpu

OK, INVALID_ARG = 0, 1
GATHER_LANES = 64       # the block of k_p3_gather: its loops step by the block


def _header_constants():
    """The integer `constexpr` constants of p3_kernels.h, read from the source so that the shapes follow them."""
    vals = {}
    for line in open(os.path.join(ROOT, "plonky2.5_amd", "csrc", "p3_kernels.h")):
        m = re.match(r"constexpr\s+(?:int|size_t|unsigned|uint32_t)\s+(\w+)\s*=\s*([^;]+);", line)
        if m:
            try:
                vals[m.group(1)] = int(eval(re.sub(r"(\d)u\b", r"\1", m.group(2)), {"__builtins__": {}}, vals))
            except (NameError, SyntaxError, TypeError):
                pass                # not plain integer arithmetic: none of the constants used here
    return vals


_K = _header_constants()
COOP_MAX, TOP_NODES, TAIL_LOG, MAX_LIVE = (_K[n] for n in ("P3_TREE_COOP_MAX", "P3_TREE_TOP_NODES", "P3_TAIL_LOG", "P3_MAX_LIVE"))


def _host(gpu, air, trace, q, pow_bits, log_blowup=1, pow_start=0):
    """(words, OK) or (None, status) of the host prover."""
    try:
        return gpu.p3_prove_air(air, trace, num_queries=q, pow_bits=pow_bits, pow_start=pow_start, log_blowup=log_blowup)[0], OK
    except gpu.P25Error as e:
        return None, e.status


def _same(got, want, what=""):
    bad = np.nonzero(got != want)[0]
    assert got.shape == want.shape and bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, first at {bad[:8].tolist()}"


def _check_one(gpu, air, trace, q, pow_bits, log_blowup=1, pow_start=0):
    log_n = int(trace.shape[0]).bit_length() - 1
    pr = gpu.P3Prover(air, log_n, log_blowup, q, pow_bits)
    got, st = pr.prove(trace, pow_starts=[pow_start])
    want, host_st = _host(gpu, air, trace, q, pow_bits, log_blowup, pow_start)
    assert host_st == OK and st.tolist() == [OK]
    _same(got[0], want)
    pr.close()
    return got[0], pr.num_inputs


def _tree_forms(h, G):
    """The launch form of every level of a tree over h leaf digests in a group of G proofs, by build_tree's rule."""
    forms, level, log_h = [], 0, h.bit_length() - 1
    while level < log_h and (h >> (level + 1)) * G > COOP_MAX:      # k_p3_tree_level
        forms.append("lane")
        level += 1
    while level < log_h and (h >> (level + 1)) > TOP_NODES:         # k_p3_tree_coop, one level
        forms.append("coop")
        level += 1
    return forms + ["top"] * (log_h - level)                        # k_p3_tree_coop, the rest in one workgroup


# ---------------------------------------------------------------------------------------------------------------------
# 1. one lane per node, long gather loops
# ---------------------------------------------------------------------------------------------------------------------
def test_per_lane_level_and_long_paths_one_proof(gpu):
    """Fibonacci at the smallest L whose trace tree has a per-lane level with ONE proof and whose paths pass 64 words."""
    log_blowup = 4
    L = max(COOP_MAX.bit_length() + 1, GATHER_LANES // 4 + 2)
    log_n = L - log_blowup
    assert log_n <= 14, "a threshold moved: this shape would be larger than the suite may run"
    N2 = 1 << L
    # trace and quotient trees over N2 leaves: level 0 on k_p3_tree_level, level 1 is the EQUALITY case (cooperative)
    assert _tree_forms(N2, 1)[:2] == ["lane", "coop"] and (N2 >> 2) == COOP_MAX
    assert "top" in _tree_forms(N2, 1)
    # the tree of FRI round 0 over N2 / 2 leaves starts on the equality case too
    assert _tree_forms(N2 >> 1, 1)[0] == "coop"
    # Merkle paths of 4 L words and the FRI path of round 0, 4 (L - 1) words: a second trip of the gather's loops
    assert 4 * L > GATHER_LANES and 4 * (L - 1) > GATHER_LANES
    # the FRI rounds in front of the workgroup tail (0 .. 7) are launches of their own; both halves of the blowup-4 LDE
    # are two-pass transforms
    assert min(log_n, L - TAIL_LOG) == L - TAIL_LOG >= 2 and log_n >= 11
    _check_one(gpu, gpu.Air.fibonacci(), air_cases.fib_trace(log_n), 3, 4, log_blowup)


@pytest.fixture(scope="module")
def squares5_2048(gpu):
    """Five `squares` traces of 2^11 rows and the host's proof of each from its own pow_start: computed once."""
    air = air_cases.squares(gpu)
    traces = np.stack([air_cases.squares_trace(11, seed=s) for s in range(1, 6)])
    want = np.stack([_host(gpu, air, traces[i], 3, 4, pow_start=POW_STARTS[i])[0] for i in range(5)])
    want.setflags(write=False)
    return air, traces, want


@pytest.mark.parametrize("extra", [0, 1])
def test_per_lane_level_under_a_batch(gpu, squares5_2048, extra):
    """One group of G and of G + 1 proofs, G the batch at which level 1 of the trace tree sits ON the threshold."""
    air, traces, want = squares5_2048
    log_n, N2 = 11, 1 << 12
    G0 = COOP_MAX // (N2 >> 2)
    assert G0 >= 2 and G0 * (N2 >> 2) == COOP_MAX and G0 + 1 <= 128, "a threshold moved: no batch of this shape sits on it"
    G = G0 + extra
    forms, fri0 = _tree_forms(N2, G), _tree_forms(N2 >> 1, G)
    if extra == 0:      # level 0 per-lane in blocks with blockIdx.y > 0, level 1 exactly on the threshold: cooperative
        assert forms[:2] == ["lane", "coop"] and fri0[0] == "coop"
    else:               # level 1 per-lane too, and level 0 of the tree of FRI round 0
        assert forms[:3] == ["lane", "lane", "coop"] and fri0[:2] == ["lane", "coop"]
    assert min(log_n, 12 - TAIL_LOG) >= 1        # FRI round 0 is a launch of its own
    pick = np.arange(G) % 5
    pr = gpu.P3Prover(air, log_n, 1, 3, 4)       # about 1.5 MB of scratch per proof: one group under the default budget
    got, st = pr.prove(traces[pick], pow_starts=np.array(POW_STARTS, dtype=np.uint64)[pick])
    assert st.tolist() == [OK] * G
    for i in range(G):
        _same(got[i], want[pick[i]], f"proof {i}")
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the LDE at every blowup: two-pass transforms with several chunks, and the smallest transforms
# ---------------------------------------------------------------------------------------------------------------------
def _two_pass_case(p25, name):
    """(air, trace, log_blowup, quotient chunks)"""
    if name == "cubic/b2":          # LDE step 2
        return air_cases.cubic(p25), air_cases.cubic_trace(11), 2, 2
    if name == "quartic_map/b2":    # step 1
        air, par = air_cases.quartic_map(p25, 6)
        return air, air_cases.quartic_map_trace(par, 11), 2, 4
    if name == "quintic_selector/b3":
        air, par = air_cases.quintic_selector(p25, 8)
        return air, air_cases.quintic_selector_trace(par, 11), 3, 4
    if name == "sextic/b3":
        return _sextic(p25, 11, 5, 3), _sextic_trace(11, 5, 3, 11), 3, 8
    assert name == "cubic/n12/b4"   # two ntt_lde_bitrev calls, each a two-pass transform
    return air_cases.cubic(p25), air_cases.cubic_trace(12), 4, 2


@pytest.mark.parametrize("name", ["cubic/b2", "quartic_map/b2", "quintic_selector/b3", "sextic/b3", "cubic/n12/b4"])
def test_two_pass_transform_at_every_blowup(gpu, name):
    air, trace, log_blowup, chunks = _two_pass_case(gpu, name)
    assert trace.shape[0] >= 1 << 11        # the transform of 2^11 points and more runs in two passes
    pr = gpu.P3Prover(air, int(trace.shape[0]).bit_length() - 1, log_blowup, 3, 4)
    assert 1 << pr.config.log_quotient_degree == chunks
    pr.close()
    _check_one(gpu, air, trace, 3, 4, log_blowup)


@pytest.mark.parametrize("log_n,log_blowup", [(1, 2), (1, 4), (2, 3), (2, 4), (3, 2)])
def test_smallest_transforms_at_every_blowup(gpu, log_n, log_blowup):
    _check_one(gpu, gpu.Air.fibonacci(), air_cases.fib_trace(log_n), 3, 4, log_blowup)


def test_width_above_the_gathers_block(gpu):
    """70 columns: the second trip of the column loop of k_p3_gather, 18 permutations per leaf, 142 opening jobs."""
    width = 70
    assert width > GATHER_LANES and -(-width // 4) == 18 and 2 * width + 2 == 142
    air, coef = air_cases.random_recurrence(gpu, 40 + width, width)
    _check_one(gpu, air, air_cases.random_recurrence_trace(coef, 4), 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# 3. proof of work
# ---------------------------------------------------------------------------------------------------------------------
def test_pow_many_trips_per_lane(gpu):
    """18 bits: a window of 2^24 candidates over 2^16 lanes; the expected witness is 2^18 candidates in, four trips."""
    _check_one(gpu, gpu.Air.fibonacci(), air_cases.fib_trace(3), 3, 18)


def test_pow_last_candidate_below_p(gpu):
    """No bits asked and the search started at p - 1: one candidate, the last canonical word, and it is the witness."""
    q, L, W = 3, 4, 3
    got, ni = _check_one(gpu, gpu.Air.fibonacci(), air_cases.fib_trace(3), q, 0, pow_start=P - 1)
    assert int(got[ni - 1 - q * (W + 4 * L + 2 + 4 * L)]) == P - 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. generated DAGs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_degree,log_blowup", air_cases.DAG_CLASSES)
@pytest.mark.parametrize("seed", air_cases.DAG_SEEDS)
def test_random_dag(gpu, seed, max_degree, log_blowup):
    air, trace = air_cases.dag_case(gpu, seed, max_degree)
    q, pb = air_cases.DAG_QUERIES, air_cases.DAG_POW_BITS
    bad = air_cases.bump(trace, *air_cases.DAG_BAD_CELL)
    pr = gpu.P3Prover(air, air_cases.DAG_LOG_N, log_blowup, q, pb)
    got, st = pr.prove(np.stack([trace, bad]))
    pr.close()
    want, host_st = _host(gpu, air, trace, q, pb, log_blowup)
    assert host_st == OK and st[0] == OK
    _same(got[0], want)
    want_bad, host_bad = _host(gpu, air, bad, q, pb, log_blowup)
    assert st[1] == host_bad
    if host_bad == OK:
        _same(got[1], want_bad, "incremented cell")
    else:
        assert not got[1].any()


def test_oracle_verifier_circuit_accepts_a_dag_proof(gpu, oracle):
    air, trace = air_cases.dag_case(gpu, 3, 3)
    pr = gpu.P3Prover(air, air_cases.DAG_LOG_N, 1, air_cases.DAG_QUERIES, air_cases.DAG_POW_BITS)
    got, st = pr.prove(trace)
    assert st.tolist() == [OK]
    oc = oracle.load_circuit(gpu.Circuit.build_p3_verifier_air(pr.config, air).to_blob())
    assert oc.witness(got[0], seed=0)[1] == 0
    bad = got[0].copy()
    bad[10] = (int(bad[10]) + 1) % P
    assert oc.witness(bad, seed=0)[1] == 4


# ---------------------------------------------------------------------------------------------------------------------
# 6. every slot of the register program
# ---------------------------------------------------------------------------------------------------------------------
def test_largest_accepted_live_chain(gpu):
    """The longest chain p25_p3_prover_create takes (tests/test_p3_prover_dev_abi_cpu.py::test_live_chain_boundary pins it
    to P3_MAX_LIVE slots): found here by asking, then proved."""
    def accepted(m):
        try:
            gpu.P3Prover(air_cases.live_chain(gpu, m), 3, 1, 3, 4).close()
            return True
        except gpu.P25Error:
            return False
    m = max(m for m in range(1, 2 * MAX_LIVE) if accepted(m))
    assert not accepted(m + 1)
    _check_one(gpu, air_cases.live_chain(gpu, m), air_cases.live_chain_trace(m, 3), 3, 4)


def test_slot_churn(gpu):
    """Several hundred arithmetic nodes through a handful of slots (tests/test_p3_prover_dev_abi_cpu.py::
    test_slots_go_back_on_last_use): every slot is overwritten many times, by values read as either operand."""
    air, y = air_cases.slot_churn(gpu)
    _check_one(gpu, air, air_cases.slot_churn_trace(air, y, 3), 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# 7. verdicts cell by cell; constant traces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def squares_cells(gpu):
    """`squares` on 8 rows: the trace, the 24 traces with one cell incremented, the host's words (None = refused)."""
    air, trace = air_cases.squares(gpu), air_cases.squares_trace(3)
    bad = np.stack([air_cases.bump(trace, r, c) for r in range(8) for c in range(3)])
    host = [_host(gpu, air, t, 3, 4) for t in bad]
    return air, trace, bad, host, _host(gpu, air, trace, 3, 4)[0]


def test_every_single_cell_increment(gpu, squares_cells):
    air, _trace, bad, host, _want = squares_cells
    refused = sum(st != OK for _w, st in host)
    assert (refused, len(host) - refused) == (17, 7)       # the free cells: y on rows 0 .. 6
    assert [i for i, (_w, st) in enumerate(host) if st == OK] == [3 * r + 2 for r in range(7)]
    pr = gpu.P3Prover(air, 3, 1, 3, 4)
    got, st = pr.prove(bad)
    for i, (words, host_st) in enumerate(host):
        assert st[i] == host_st, f"cell {divmod(i, 3)}"
        if host_st == OK:
            _same(got[i], words, f"cell {divmod(i, 3)}")
        else:
            assert not got[i].any()
    one, st1 = pr.prove(bad[3 * 7 + 2])     # alone: the last row's y, pinned by the last-row constraint only
    assert st1.tolist() == [INVALID_ARG] and not one.any()
    pr.close()


def test_failed_rows_between_untouched_neighbours(gpu, squares_cells):
    """The 24 between untouched traces, into a pre-filled array with padding behind every row: a failed row is zeros, every
    other row is the host's, the padding keeps what it held."""
    air, trace, bad, host, want = squares_cells
    batch = np.empty((48,) + trace.shape, dtype=np.uint64)
    batch[0::2], batch[1::2] = trace, bad
    pr = gpu.P3Prover(air, 3, 1, 3, 4)
    got, st = pr.prove(batch, input_stride=pr.num_inputs + 3)
    ni = pr.num_inputs
    assert not got[:, ni:].any()
    for i in range(24):
        assert st[2 * i] == OK and st[2 * i + 1] == host[i][1]
        _same(got[2 * i, :ni], want, f"neighbour {2 * i}")
        if host[i][1] == OK:
            _same(got[2 * i + 1, :ni], host[i][0], f"row {2 * i + 1}")
        else:
            assert not got[2 * i + 1].any()
    pr.close()


@pytest.mark.parametrize("y0", [0, 1])
def test_constant_trace(gpu, y0):
    got, _ni = _check_one(gpu, air_cases.constant_pair(gpu, y0), air_cases.constant_pair_trace(y0, 5), 3, 4)
    if y0 == 0:
        # zero by construction: the quotient's opening at zeta (2 words) and its value at every query (3 x 2), the
        # sibling value of 5 FRI rounds per query (3 x 5 x 2), the final polynomial (2)
        assert np.count_nonzero(got == 0) >= 2 + 6 + 30 + 2
