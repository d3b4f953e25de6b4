"""CPU: the boundary-valued traces of tests/air_cases_edge.py and the host prover's answers on them.

tests/test_gpu_p3_edge_values.py compares the device prover with the host prover (p3_prove_air) on these traces.  Here
    the traces     built in Python integers, satisfy their AIRs row by row, the constraints evaluated in Python integers
    the host       its proof of every family and fill at 2^3 rows (2^4 for the LogUp AIRs) is accepted by the plain-Python
                   verifier (tests/p3_verify_model.py, p3_aux_model.py), and one proof per family by the oracle's witness of
                   the reference's verifier circuit
so that the host's words on this data are an independently checked quantity."""
import types

import numpy as np
import pytest

import air_cases_edge as edge
import edge_values as ev
import p3_aux_model as AM
import p3_verify_cases as pc
import p3_verify_model as M
from conftest import P
from test_p3_verify_lanes_cpu import _build_driver

QUERIES, POW_BITS = 3, 4


def _prove(p25, air, trace, log_blowup, pv=None, q=QUERIES, pow_bits=POW_BITS):
    return p25.p3_prove_air(air, trace, num_queries=q, pow_bits=pow_bits, log_blowup=log_blowup, threads=1, public_values=pv)


# ---- the traces -----------------------------------------------------------------------------------------------------------
def test_fills_are_boundary_valued_and_canonical():
    assert len(edge.FILL_NAMES) == 11 and set(ev.GENERATORS) <= set(edge.FILL_NAMES)
    for name, fill in edge.FILLS.items():
        col = fill(64, 5)
        assert col.dtype == np.uint64 and col.shape == (64,) and (col < np.uint64(P)).all(), name
    pairs = edge.fill_pairs()
    assert len(pairs) == 22 and {a for _n, a, _b in pairs} == {b for _n, _a, b in pairs} == set(edge.FILL_NAMES)
    assert len(edge.constant_pairs()) == len(ev.EDGE) ** 2 == 400


@pytest.mark.parametrize("log_n", [3, 6])
@pytest.mark.parametrize("family", list(edge.FAMILIES))
def test_traces_satisfy_their_constraints_row_by_row(p25, family, log_n):
    air = edge.FAMILIES[family][0](p25)
    named = edge.traces(family, log_n)
    assert len(named) == (11 if family == "free_pow5" else 22)
    for name, trace in named:
        assert trace.shape == (1 << log_n, air.width) and (trace < np.uint64(P)).all()
        assert edge.check_rows(air, trace) is None, (family, name)
    # and the check does bite: one derived cell incremented
    bad = named[0][1].copy()
    bad[2, air.width - 1] = (int(bad[2, air.width - 1]) + 1) % P
    assert edge.check_rows(air, bad) is not None


def test_constant_traces_satisfy_free_ops(p25):
    air = edge.free_ops(p25)
    traces = edge.free_ops_constant_traces(1)
    assert traces.shape == (len(ev.EDGE) ** 2, 2, 5)
    for pair, trace in zip(edge.constant_pairs(), traces):
        assert tuple(int(v) for v in trace[0, :2]) == pair and (trace[0] == trace[1]).all()
        assert edge.check_rows(air, trace) is None, pair


# ---- the host prover against the models -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(edge.FAMILIES))
def test_host_proofs_of_every_fill_pass_the_model(p25, oracle, family):
    make_air, _t, degree, log_blowups = edge.FAMILIES[family]
    air = make_air(p25)
    for log_blowup in log_blowups:
        for k, (name, trace) in enumerate(edge.traces(family, 3)):
            words, cfg = _prove(p25, air, trace, log_blowup)
            assert 1 << cfg.log_quotient_degree == {2: 1, 3: 2, 5: 4}[degree]
            assert (words < np.uint64(P)).all()
            assert M.verify(oracle, air, cfg, words) == M.OK, (family, log_blowup, name)
            if k == 0:              # one proof per family and blowup through the oracle's verifier circuit, and not a changed one
                assert pc.oracle_accepts(p25, oracle, air, cfg, words)
                bad = pc.flipped(words, M.Shape(cfg).o_trace_local)
                assert M.verify(oracle, air, cfg, bad) != M.OK and not pc.oracle_accepts(p25, oracle, air, cfg, bad)


def test_host_proofs_of_constant_pairs_pass_the_model(p25, oracle):
    """Every 23rd pair and the four corners of EDGE x EDGE at 2^3 rows, 2 queries, no proof of work (the shape of the GPU
    test's 400-proof batch); the quotient's openings are zero."""
    air = edge.free_ops(p25)
    pairs, traces = edge.constant_pairs(), edge.free_ops_constant_traces(3)
    n = len(pairs)
    for i in sorted(set(range(0, n, 23)) | {0, len(ev.EDGE) - 1, n - len(ev.EDGE), n - 1}):
        words, cfg = _prove(p25, air, traces[i], 1, q=2, pow_bits=0)
        s = M.Shape(cfg)
        assert not words[s.o_chunks:s.o_chunks + 4].any() and not words[s.o_final_poly:s.o_final_poly + 2].any()
        assert M.verify(oracle, air, cfg, words) == M.OK, pairs[i]
    assert pc.oracle_accepts(p25, oracle, air, cfg, words)


def test_the_zero_proof_of_the_verifier_sweep(p25, oracle):
    """free_ops, the constant trace of (p - 1, 2^32 - 1) at 2^2 rows and 2 queries: accepted by the model and the circuit; with
    a flipped final-polynomial word, by neither."""
    air = edge.free_ops(p25)
    trace = edge.free_ops_constant_traces(2)[edge.constant_pairs().index((P - 1, (1 << 32) - 1))]
    words, cfg = _prove(p25, air, trace, 1, q=2, pow_bits=0)
    s = M.Shape(cfg)
    assert words.size == s.num_inputs == 137
    assert M.verify(oracle, air, cfg, words) == M.OK and pc.oracle_accepts(p25, oracle, air, cfg, words)
    bad = pc.flipped(words, s.o_final_poly)
    assert M.verify(oracle, air, cfg, bad) == M.FINAL_POLY and not pc.oracle_accepts(p25, oracle, air, cfg, bad)


# ---- the verifier's lane functions, compiled for the host --------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes(p25, tmp_path_factory):
    """tests/native/p3_verify_lanes.cpp: p3_verify_lanes.h and run_air in F_p^2, lane by lane in plain loops."""
    return _build_driver(p25, tmp_path_factory, "p3_verify_lanes_edge", [])


def test_host_lanes_accept_every_constant_pair(p25, lanes):
    """All 400 proofs of the GPU test's batch through the identity lane: the opened values are (u, 0), (v, 0), ... so the
    interpreter multiplies, adds and subtracts exactly the pair."""
    air = edge.free_ops(p25)
    words = [_prove(p25, air, t, 1, q=2, pow_bits=0)[0] for t in edge.free_ops_constant_traces(3)]
    case = types.SimpleNamespace(air=air, log_n=3, log_blowup=1, queries=2, pow_bits=0)
    got = lanes(case, words)
    assert got == [M.OK] * 400, [edge.constant_pairs()[i] for i, g in enumerate(got) if g != M.OK][:5]


@pytest.mark.parametrize("family", list(edge.FAMILIES))
def test_host_lanes_accept_every_fill_and_match_the_model_on_flips(p25, oracle, lanes, family):
    make_air, _t, _degree, log_blowups = edge.FAMILIES[family]
    air = make_air(p25)
    for log_blowup in log_blowups:
        proved = [_prove(p25, air, t, log_blowup) for _name, t in edge.traces(family, 3)]
        words, cfg = [w for w, _cfg in proved], proved[0][1]
        case = types.SimpleNamespace(air=air, log_n=3, log_blowup=log_blowup, queries=QUERIES, pow_bits=POW_BITS)
        assert lanes(case, words) == [M.OK] * len(words), (family, log_blowup)
        flips = [w for _pos, w in pc.all_flips(words[0])][::5]          # of the first fill's proof, at this blowup
        assert lanes(case, flips) == [M.verify(oracle, air, cfg, w) for w in flips], (family, log_blowup)


def test_host_lanes_on_every_flip_of_the_zero_proof(p25, oracle, lanes):
    air = edge.free_ops(p25)
    trace = edge.free_ops_constant_traces(2)[edge.constant_pairs().index((P - 1, (1 << 32) - 1))]
    words, cfg = _prove(p25, air, trace, 1, q=2, pow_bits=0)
    case = types.SimpleNamespace(air=air, log_n=2, log_blowup=1, queries=2, pow_bits=0)
    proofs = [words] + [w for _pos, w in pc.all_flips(words)] + [pc.with_word(words, pos, P) for pos in range(0, words.size, 3)]
    want = [M.verify(oracle, air, cfg, w) for w in proofs]
    assert lanes(case, proofs) == want and want[0] == M.OK and M.MALFORMED in want and M.FINAL_POLY in want


# ---- F_p^2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["edge_range", "edge_pvper"])
def test_host_logup_proofs_on_boundary_words_pass_the_model(p25, oracle, kind):
    log_n = edge.EXT_LOG_SMALL
    n = 1 << log_n
    proved = []
    for seed in (0, 1, 2):
        air, trace, pv = edge.ext_case(p25, kind, log_n, seed)
        assert (trace < np.uint64(P)).all() and set(int(v) for v in trace[:, 0]) <= set(ev.EDGE)
        words, cfg = _prove(p25, air, trace, 1, pv)          # status 0: no zero denominator
        key = None if air.preprocessed is None else p25.p3_preprocessed_commit(air.preprocessed, 1, threads=1)
        pw = 0 if air.preprocessed is None else int(air.preprocessed.shape[1])
        shape = AM.Shape(cfg, pw, 1)
        assert words.size == shape.num_inputs + air.n_public
        assert AM.verify(oracle, air, cfg, words, key) == AM.OK, (kind, seed)
        # the trace builder, in Python integers: under this proof's challenge the lookups and the table's multiplicities
        # cancel, sum_i 1 / (g - f_i) = sum_i m_i / (g - t_i) in F_p^2 ...
        g = AM.challenges_of(oracle, air, words, cfg, key)[0]
        if kind == "edge_pvper":
            g = AM.e_add(g, AM.e(int(pv[0])))
            table = [int(edge.EDGE_PERIODIC[i % edge.EDGE_PERIODIC.size]) for i in range(n)]
            assert int(trace[0, 0]) == int(pv[1])             # the first-row constraint
        else:
            table = [int(v) for v in air.preprocessed[:, 0]]
        looked = (0, 0)
        for i in range(n):
            looked = AM.e_add(looked, AM.e_inv(AM.e_sub(g, AM.e(int(trace[i, 0])))))
            looked = AM.e_sub(looked, AM.e_mul(AM.e(int(trace[i, 1])), AM.e_inv(AM.e_sub(g, AM.e(table[i])))))
        assert looked == (0, 0), (kind, seed)
        # ... and the model's running sums of the AIR's own num / den close: the last sum and the last row's term give zero
        pvs = [int(v) for v in pv] if pv is not None else []
        sums = AM.running_sums(air, trace, pvs, AM.challenges_of(oracle, air, words, cfg, key))
        f, m = int(trace[n - 1, 0]), int(trace[n - 1, 1])
        gf, gt = AM.e_sub(g, AM.e(f)), AM.e_sub(g, AM.e(table[n - 1]))
        last = AM.e_mul(AM.e_sub(AM.e_mul(AM.e(m), gf), gt), AM.e_inv(AM.e_mul(gt, gf)))
        assert sums[0] == [(0, 0)] and len(sums) == n and AM.e_add(sums[n - 1][0], last) == (0, 0), (kind, seed)
        proved.append((air, words, cfg, key, shape))
    air, words, cfg, key, shape = proved[-1]
    oc = oracle.load_circuit(p25.Circuit.build_p3_verifier_air(cfg, air).to_blob())
    assert oc.witness(words, seed=3)[1] == 0
    bad = words.copy()
    bad[shape.o_aux_local] = (int(bad[shape.o_aux_local]) + 1) % P
    assert AM.verify(oracle, air, cfg, bad, key) != AM.OK and oc.witness(bad, seed=3)[1] == 4


def test_the_logup_tables_hold_the_boundary_words():
    assert [int(v) for v in edge.edge_table(5)[:, 0]] == [ev.EDGE[i % len(ev.EDGE)] for i in range(32)]
    assert set(int(v) for v in edge.edge_table(5)[:, 0]) == set(ev.EDGE)
    trace = edge.edge_range_trace(4)
    assert int(trace[:, 1].astype(object).sum()) == 16      # the multiplicities count the 16 draws
