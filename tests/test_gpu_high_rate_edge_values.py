"""GPU: the stage kernels at FRI rates 4..8 on boundary-valued Goldilocks operands (tests/edge_values.py).

tests/test_gpu_edge_values.py stops at rate 3; the k_ntt_tile instantiations that rates 4..8 added -- more than 8 cosets in
one pass-1 launch, pass 1 with the factored pre-scale, the NTT_FACTOR_LOG / NTT_PRE_TABLE_LOG switch of ntt_lde_bitrev --
and the quotient on the 8n-point sub-coset had seen uniform words and satisfied witnesses only (tests/test_gpu_high_rate.py).
Here they get the inputs of that suite: every word on or next to a boundary of the lazy arithmetic, and structured columns
that keep the intermediates there.

Rule of tests/test_gpu_edge_values.py: every comparison exact, every output word canonical (`_same`).  References: Python
integers (log_n 3 and 6), closed forms at 2^20 and 2^21 points, the oracle elsewhere -- whose LDE at these rates
tests/test_edge_values_cpu.py holds to the Python forms on the same columns."""
import functools

import numpy as np
import pytest

import edge_values as ev
import high_rate as hr
from test_gpu_edge_values import (NONCANONICAL_RULE, PU, _boundary_challenges, _one_row_per_gate_kind, _reduces_or_refuses, _same,
                                  _whole_matrices, _with_noncanonical)
from test_gpu_high_rate import LDE_CASES
from verify_cases import reference_gates_inputs

pytestmark = pytest.mark.gpu


_NTT = ev.ntt_source_constants()        # a threshold that moves takes the rule below with it; the shapes then fail their preconditions
FACTOR_LOG, PRE_TABLE_LOG, TWO_PASS_LOG = _NTT["NTT_FACTOR_LOG"], _NTT["NTT_PRE_TABLE_LOG"], _NTT["TWO_PASS_LOG"]


def _factored(log_n, rate):
    """ntt_lde_bitrev's rule for the two factor tables of the coset pre-scale."""
    return log_n >= TWO_PASS_LOG and (log_n > FACTOR_LOG or log_n + rate > PRE_TABLE_LOG)


# ---- 1. LDE vs Python integers ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _naive(log_n, from_coeffs):
    """[(rate, name, input column, coefficients, LDE)] in Python integers, computed once."""
    rates, cols = ev.high_rate_naive_columns(log_n, 200 + log_n)
    out = []
    for name, col in cols.items():
        coeffs = col if from_coeffs else ev.intt_naive(col)
        out += [(rate, name, col, coeffs, ev.coset_lde_naive(coeffs, rate)) for rate in rates]
    return out


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("log_n", [3, 6])
def test_lde_commit_vs_python_integers(gpu, log_n, from_coeffs):
    want = _naive(log_n, from_coeffs)
    for rate in sorted({w[0] for w in want}):
        rows = [w for w in want if w[0] == rate]
        cg, lg, _cap = gpu.lde_commit(np.stack([w[2] for w in rows]), rate, 0, from_coeffs)
        for k, (_r, name, _col, coeffs, lde) in enumerate(rows):
            _same(cg[k], coeffs, ("coefficients", name, log_n, rate))
            _same(lg[k], lde, ("lde", name, log_n, rate))


# ---- 2. LDE vs the oracle at the form boundaries ------------------------------------------------------------------------
ORACLE_CASES = [(log_n, rate) for log_n, _cols, rate in LDE_CASES if log_n + rate <= 20 and log_n < 16]     # (16, 4): item 3


def test_oracle_cases_sit_on_the_form_boundaries():
    assert ORACLE_CASES == [(10, 4), (10, 8), (11, 4), (11, 8), (12, 8), (12, 5), (13, 6)]
    assert [(ln, r) for ln, r in ORACLE_CASES if ln < TWO_PASS_LOG] == [(10, 4), (10, 8)]            # single pass, 16 / 256 cosets
    assert 11 + 8 == PRE_TABLE_LOG and not _factored(11, 8) and not _factored(11, 4)                 # the last unfactored size
    assert _factored(12, 8) and 12 <= FACTOR_LOG                                                     # factored at a small size
    assert not _factored(12, 5) and not _factored(13, 6)                                             # radix remainders, unfactored
    assert not _factored(16, 3) and _factored(16, 4) and 17 > FACTOR_LOG and _factored(17, 4)        # item 3's two shapes


@pytest.mark.parametrize("log_n,rate", ORACLE_CASES)
def test_lde_commit_forms_vs_oracle_on_edge_columns(gpu, oracle, log_n, rate):
    """From values and from coefficients; the oracle's coefficients of the first are the input of the second, whose LDE and
    cap are therefore the same: one oracle LDE per case.  All ten columns below 2^18 points, four from there (the oracle's
    Merkle tree over wider leaves is what would make a case take 7 to 15 s: ev.HIGH_RATE_ORACLE_KEEP)."""
    cols = ev.high_rate_oracle_columns(log_n, rate, 500 + 16 * log_n + rate)
    vals = np.stack(list(cols.values()))
    co, lo, capo = oracle.lde_commit(vals, rate, 4, False)
    for from_coeffs, given in ((False, vals), (True, co)):
        cg, lg, capg = gpu.lde_commit(given, rate, 4, from_coeffs)
        what = (list(cols), log_n, rate, from_coeffs)
        _same(cg, co, ("coefficients",) + what)
        _same(lg, lo, ("lde",) + what)
        _same(capg, capo, ("cap",) + what)


# ---- 3. closed forms at 2^20 and 2^21 points ----------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,rate", [(16, 4), (17, 4)])
def test_full_size_lde_of_structured_columns(gpu, log_n, rate):
    """(16, 4): the constant-shape instantiation of pass 2 behind a pass 1 with the factored pre-scale (factored by the
    table's size); (17, 4): factored by the transform's size.  No oracle: the closed forms of ev.high_rate_closed_forms."""
    assert log_n >= TWO_PASS_LOG and _factored(log_n, rate) and (log_n > FACTOR_LOG) == (log_n == 17)
    values_in, coeffs_in = ev.high_rate_closed_forms(log_n, rate)
    cg, lg, _cap = gpu.lde_commit(np.stack([v for _n, v, _c, _l in values_in]), rate, 4)
    for k, (name, _v, coeffs, lde) in enumerate(values_in):
        _same(cg[k], coeffs, ("coefficients", name, log_n, rate))
        if lde is not None:
            _same(lg[k], lde, ("lde", name, log_n, rate))
    assert (lg < PU).all()
    given = np.stack([c for _n, c, _l in coeffs_in])
    cg, lg, _cap = gpu.lde_commit(given, rate, 4, from_coeffs=True)
    _same(cg, given, "coefficients handed back")
    for k, (name, _c, lde) in enumerate(coeffs_in):
        _same(lg[k], lde, ("lde of", name, log_n, rate))


# ---- 4. the layout identity the quotient kernel rests on ----------------------------------------------------------------
@pytest.mark.parametrize("log_n", [11, 12])
def test_lde_prefix_is_the_rate_3_lde_on_edge_columns(gpu, log_n):
    """The first 8n words of a bit-reversed LDE column of any rate above 3 are the rate-3 column (whose words
    tests/test_gpu_edge_values.py pins), from values and from coefficients.  From coefficients the boundary words themselves
    are what the coset pre-scale multiplies -- in the oracle cases above the LDE's input is the interpolant's coefficients,
    uniform-looking words -- and at log_n 12 rate 8 takes the factored pre-scale, whose two products then see every member
    of EDGE."""
    assert log_n >= TWO_PASS_LOG
    assert (log_n, [r for r in (4, 5, 6, 7, 8) if _factored(log_n, r)]) in ((11, []), (12, [8]))
    cols = ev.columns(1 << log_n, 77)
    vals = np.stack(list(cols.values()))
    for from_coeffs in (False, True):
        _c, l3, _cap = gpu.lde_commit(vals, 3, 4, from_coeffs)
        assert (l3 < PU).all()
        for rate in (4, 5, 6, 7, 8):
            _c, lr, _cap = gpu.lde_commit(vals, rate, 4, from_coeffs)
            _same(lr[:, :8 << log_n], l3, ("prefix", list(cols), rate, from_coeffs))


# ---- 5. words >= p ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("rate", [4, 8])
@pytest.mark.parametrize("log_n", [6, 11])
def test_noncanonical_words_lde_commit(gpu, oracle, log_n, rate, from_coeffs):
    n = 1 << log_n
    raw, red = _with_noncanonical(ev.edge(3 * n, 9))
    raw, red = raw.reshape(3, n), red.reshape(3, n)
    want = oracle.lde_commit(red, rate, 2, from_coeffs)
    got = _reduces_or_refuses(gpu, lambda a: gpu.lde_commit(a, rate, 2, from_coeffs), raw, want,
                              ("lde_commit", log_n, rate, from_coeffs))
    assert got == NONCANONICAL_RULE["lde_commit"]


# ---- 6. partial products and the quotient on the 8n-point sub-coset ------------------------------------------------------
GADGET14_KINDS = (1, 2, 4, 5, 6, 9, 10)     # the gate kinds the reference-gates gadget holds


@pytest.fixture(scope="module", params=[4, 8])
def gadget14(request, gpu, oracle):
    rate = request.param
    c = gpu.Circuit.build_gadget(14, 0, (rate, hr.QUERIES[rate], 16))
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF), seed=4)
    assert st == 0, msg
    assert c.config.as_tuple() == (rate, hr.QUERIES[rate], 16)
    yield c, oc, wires, f"gadget 14 at rate {rate}"
    c.close()


@pytest.fixture(scope="module")
def small_rate4(gpu, oracle):
    """The 2^10-row plonky3-verifier circuit rebuilt by blob rewrite to rate 4: a 2^13-point inverse transform from the
    prefix of 2^14-point LDE columns."""
    inp, cfg = gpu.p3_prove_fibonacci(3, 3, 4)
    std = gpu.Circuit.build_p3_verifier(cfg)
    c = gpu.Circuit.from_blob(hr.rewrite_config(std.to_blob(), 4, hr.QUERIES[4]))
    assert int(c.info.degree_bits) == 10 and c.config.as_tuple() == (4, 21, 16)
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(inp, seed=5)
    assert st == 0, msg
    yield c, oc, wires, "2^10 rows at rate 4"
    c.close()
    std.close()


def test_stage_kernels_on_edge_wire_matrices_gadget_14(gadget14):
    _whole_matrices(*gadget14)


def test_stage_kernels_under_boundary_challenges_gadget_14(gadget14):
    _boundary_challenges(*gadget14, witness_too=True)


def test_stage_kernels_one_edge_row_per_gate_kind_gadget_14(gadget14):
    _one_row_per_gate_kind(*gadget14, GADGET14_KINDS)


def test_stage_kernels_on_edge_wire_matrices_2_10_rows_at_rate_4(small_rate4):
    _whole_matrices(*small_rate4)


def test_stage_kernels_under_boundary_challenges_2_10_rows_at_rate_4(small_rate4):
    _boundary_challenges(*small_rate4, witness_too=True)


def test_stage_kernels_one_edge_row_per_gate_kind_2_10_rows_at_rate_4(small_rate4):
    _one_row_per_gate_kind(*small_rate4, range(1, 11))


# ---- 7. FRI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,rate,arity", [(6, 8, [4]), (10, 5, [4, 4]), (12, 4, [4, 4])])
def test_fri_prove_on_edge_polynomials(gpu, oracle, log_n, rate, arity):
    seed = ev.uniform(13, 98)
    for name, coeffs in ev.fri_polynomials(log_n).items():
        g, st = gpu.fri_prove(coeffs, rate, 4, arity, 10, hr.QUERIES[rate], seed)
        assert st == 0, name
        o = oracle.fri_prove(coeffs, rate, 4, arity, 10, hr.QUERIES[rate], seed)       # asserts its own success
        _same(g, o, ("fri_prove", name, log_n, rate))
