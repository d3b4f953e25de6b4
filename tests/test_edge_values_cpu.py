"""CPU: the boundary-valued inputs of tests/edge_values.py and its Python-integer references.

The generators are deterministic and canonical; the plain references equal the oracle on boundary data at the sizes the
naive forms can afford -- which makes the oracle's answer on such data an independently checked quantity, so that
tests/test_gpu_edge_values.py may use the oracle where Python cannot go; and the oracle accepts every input class that
module uses.  GPU twin: tests/test_gpu_edge_values.py."""
import numpy as np
import pytest

import edge_values as ev
import stage_circuits
from edge_values import EDGE, EPS, P


def test_edge_list_holds_the_boundaries():
    for v in (0, 1, 2, 3, 7, pow(7, P - 2, P), EPS - 1, EPS, EPS + 1, EPS + 2, (1 << 63) - 1, 1 << 63, (P - 1) // 2,
              (P + 1) // 2, 0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFFFF, P - (1 << 32), P - EPS, P - EPS - 1, P - 3, P - 2, P - 1):
        assert v in EDGE, hex(v)
    assert all(0 <= v < P for v in EDGE) and len(set(EDGE)) == len(EDGE)
    assert 7 * ev.INV7 % P == 1 and (1 << 64) % P == EPS
    # every half-word pattern a carry or a correction keys on
    assert {v & 0xFFFFFFFF for v in EDGE} >= {0, 1, 0xFFFFFFFF, 0xFFFFFFFE}
    assert {v >> 32 for v in EDGE} >= {0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x7FFFFFFF, 0x80000000}
    assert [v >= P for v in ev.NONCANONICAL] == [True, True, True, False] and ev.NONCANONICAL[3] == P - 1


@pytest.mark.parametrize("name", ["uniform", "edge", "high", "low", "mixed"])
def test_generators_are_deterministic_and_canonical(name):
    gen = getattr(ev, name)
    a, b, c = gen(4096, 5), gen(4096, 5), gen(4096, 6)
    assert a.dtype == np.uint64 and a.shape == (4096,)
    assert (a == b).all() and (a != c).any()
    assert (a < np.uint64(P)).all()
    assert (gen(100, 5) == a[:100]).all()                  # a prefix of the same stream


def test_generator_ranges():
    e, h, l, m = (set(int(v) for v in g(8192, 3)) for g in (ev.edge, ev.high, ev.low, ev.mixed))
    assert e == set(EDGE)
    assert set(EDGE) <= m
    assert all(P - (1 << 32) <= v < P for v in h) and len(h) > 8000
    assert all(v < 1 << 33 for v in l) and any(v >> 32 for v in l) and len(l) > 8000
    mm = [int(v) for v in ev.mixed(8192, 3)]
    assert all(v in EDGE for v in mm[0::4]) and all(v >= P - (1 << 32) for v in mm[1::4])
    assert all(v < 1 << 33 for v in mm[2::4]) and len(set(mm[3::4])) == 2048


def test_structured_fills():
    n = 64
    assert ev.const(n, P - 1).tolist() == [P - 1] * n and ev.const(n, 0).tolist() == [0] * n
    d = ev.delta(n, 5, P - 1)
    assert int(d[5]) == P - 1 and int(d.astype(object).sum()) == P - 1
    assert ev.alternating(n, P - 1, 0).tolist() == [P - 1, 0] * (n // 2)
    w = ev.root_of_unity(6)
    g = [int(v) for v in ev.geometric(n, w)]
    assert g[0] == 1 and g[1] == w and g[n // 2] == P - 1 and g[n - 1] * w % P == 1
    for fill in (ev.const(n, P - 1), d, ev.alternating(n, P - 1, 0), ev.geometric(n, w), ev.geometric(n, P - 1)):
        assert fill.dtype == np.uint64 and (fill < np.uint64(P)).all()


def _edge_columns(n):
    return {"edge": ev.edge(n, 21), "const(p-1)": ev.const(n, P - 1), "const(0)": ev.const(n, 0),
            "alternating(p-1,0)": ev.alternating(n, P - 1, 0), "delta(n-1,p-1)": ev.delta(n, n - 1, P - 1),
            "geometric(w)": ev.geometric(n, ev.root_of_unity(n.bit_length() - 1))}


@pytest.mark.parametrize("log_n", [3, 6])
def test_closed_forms_equal_the_naive_dft(log_n):
    n = 1 << log_n
    for v in (1, P - 1, EPS):
        assert (ev.intt_naive(ev.const(n, v)) == ev.intt_of_const(n, v)).all()
        for r in (0, 1, n // 2, n - 1):
            assert (ev.intt_naive(ev.delta(n, r, v)) == ev.intt_of_delta(n, r, v)).all(), (v, r)
    w = ev.root_of_unity(log_n)
    for j in (0, 1, n // 2, n - 1):
        assert (ev.intt_naive(ev.geometric(n, pow(w, j, P))) == ev.intt_of_geometric(n, j)).all(), j
    for c, k in ((P - 1, 0), (EPS, 1), (P - EPS, n - 1)):
        assert (ev.coset_lde_naive(ev.delta(n, k, c), 3) == ev.lde_of_monomial(log_n + 3, c, k)).all(), (c, k)
    assert ev.coset_points(log_n)[:2] == [7, 7 * w % P]


@pytest.mark.parametrize("log_n", [3, 6])
def test_python_dft_equals_the_oracle_on_edge_columns(oracle, log_n):
    """Naive inverse DFT and coset evaluation on 7<w>, bit-reversed, in Python integers == oracle.lde_commit, rate 3."""
    n = 1 << log_n
    cols = _edge_columns(n)
    vals = np.stack(list(cols.values()))
    for from_coeffs in (False, True):
        co, lo, _cap = oracle.lde_commit(vals, 3, 0, from_coeffs)
        for k, name in enumerate(cols):
            coeffs = vals[k] if from_coeffs else ev.intt_naive(vals[k])
            assert (co[k] == coeffs).all(), (name, from_coeffs)
            assert (lo[k] == ev.coset_lde_naive(coeffs, 3)).all(), (name, from_coeffs)


@pytest.mark.parametrize("from_coeffs", [False, True])
@pytest.mark.parametrize("log_n", [3, 6])
def test_python_dft_equals_the_oracle_on_edge_columns_at_rates_4_to_8(oracle, log_n, from_coeffs):
    """The columns, rates and Python forms of tests/test_gpu_high_rate_edge_values.py::test_lde_commit_vs_python_integers
    == oracle.lde_commit: the oracle's LDE at rates 4..8 on boundary data is an independently checked quantity too."""
    rates, cols = ev.high_rate_naive_columns(log_n, 200 + log_n)
    assert set(rates) >= {4, 8} and len(cols) >= 4
    vals = np.stack(list(cols.values()))
    for rate in rates:
        co, lo, _cap = oracle.lde_commit(vals, rate, 0, from_coeffs)
        assert lo.shape == (len(cols), 1 << (log_n + rate)) and (lo < np.uint64(P)).all()
        for k, name in enumerate(cols):
            coeffs = vals[k] if from_coeffs else ev.intt_naive(vals[k])
            assert (co[k] == coeffs).all(), (name, rate)
            assert (lo[k] == ev.coset_lde_naive(coeffs, rate)).all(), (name, rate)


@pytest.mark.parametrize("log_n,rate", [(3, 4), (3, 8), (6, 4), (6, 8)])
def test_high_rate_closed_forms_equal_the_naive_forms(log_n, rate):
    """ev.high_rate_closed_forms, the reference of the 2^20- and 2^21-point LDE tests, at sizes Python can check."""
    values_in, coeffs_in = ev.high_rate_closed_forms(log_n, rate)
    assert len(values_in) == 4 and len(coeffs_in) == 5
    for name, values, coeffs, lde in values_in:
        assert (ev.intt_naive(values) == coeffs).all(), name
        if lde is not None:
            assert (ev.coset_lde_naive(coeffs, rate) == lde).all(), name
    assert [name for name, _v, _c, lde in values_in if lde is None] == ["delta(n-1,p-1)"]
    for name, coeffs, lde in coeffs_in:
        assert (ev.coset_lde_naive(coeffs, rate) == lde).all(), name


@pytest.mark.parametrize("log_n", list(range(7)))
def test_oracle_lde_over_the_small_end_of_the_accepted_domain(oracle, log_n):
    """oracle.lde_commit == a direct DFT and Horner at 7 w^i in Python integers for log_n 0..6, every rate_bits 0..3 and
    both from_coeffs values, two polynomials each: the reference of tests/test_gpu_device_entry_points.py's sweep over
    the domain p25_lde_commit accepts, checked where the naive forms can go -- sizes 1, 2 and 4 and rate 0 included,
    which nothing ran before.  The oracle refuses none of these shapes."""
    n = 1 << log_n
    vals = np.stack([ev.edge(n, 60 + log_n), ev.uniform(n, 61 + log_n)])
    for rate in range(4):
        for from_coeffs in (False, True):
            co, lo, cap = oracle.lde_commit(vals, rate, 0, from_coeffs)
            assert lo.shape == (2, n << rate) and (lo < np.uint64(P)).all() and (cap < np.uint64(P)).all()
            for k in range(2):
                coeffs = vals[k] if from_coeffs else ev.intt_naive(vals[k])
                assert (co[k] == coeffs).all(), (log_n, rate, from_coeffs, k)
                assert (lo[k] == ev.coset_lde_naive(coeffs, rate)).all(), (log_n, rate, from_coeffs, k)
            # the cap over the leaves (lde[0..2][l])_l: a leaf of two words is its own digest, padded with zeros
            if log_n + rate == 0:
                assert cap.tolist() == [[int(lo[0, 0]), int(lo[1, 0]), 0, 0]]


def test_python_horner_equals_the_oracle_on_edge_coefficients(oracle):
    """Horner in F_p[X]/(X^2 - 7) with the scale argument of p25_eval_polys == oracle.eval_polys, 2^10 coefficients."""
    n = 1 << 10
    coeffs = np.stack([ev.edge(n, 31), ev.const(n, P - 1), ev.mixed(n, 32)])
    for pt in ev.OPENING_POINTS + [(ev.root_of_unity(10), 0), (7 * ev.root_of_unity(13) % P, 0)]:
        for scale in ev.OPENING_SCALES:
            got = oracle.eval_polys(coeffs, np.array(pt, dtype=np.uint64), scale)
            for k in range(coeffs.shape[0]):
                assert tuple(int(v) for v in got[k]) == ev.horner_ext(coeffs[k], pt, scale), (pt, scale, k)


def test_oracle_fri_accepts_the_edge_polynomials(oracle):
    seed = ev.uniform(13, 99)
    for name, coeffs in ev.fri_polynomials(10).items():
        out = oracle.fri_prove(coeffs, 3, 4, [4, 4], 8, 5, seed)
        assert out.size == 586 and (out < np.uint64(P)).all(), name


@pytest.fixture(scope="module")
def small(p25, oracle):
    return stage_circuits.build_small(p25, oracle)


@pytest.mark.parametrize("which,rate", [("small", 4), ("gadget 14", 8)])
def test_oracle_quotient_of_any_wires_does_not_depend_on_the_rate(p25, oracle, small, which, rate):
    """upstream's compute_quotient_polys interpolates the quotient on the coset of 8n points whatever the rate, and those
    points and the values of every column on them are the same at every rate >= 3: the quotient chunks of a circuit
    rewritten to rate 4 or 8 are its rate-3 chunks, for wires that satisfy nothing as for the witness.  (An interpolant
    over the whole LDE domain agrees with it for a satisfied witness only: the first run of
    tests/test_gpu_high_rate_edge_values.py found the oracle computing that one.)  The 2^10-row circuit at rate 4, the
    8-row reference-gates gadget at rate 8 (the oracle takes 10 s to load 2^10 rows at rate 8)."""
    import high_rate as hr
    from verify_cases import reference_gates_inputs
    if which == "small":
        c, oc, wires = small
    else:
        c = p25.Circuit.build_gadget(14, 0)
        oc = oracle.load_circuit(c.to_blob())
        wires, st, msg = oc.witness(reference_gates_inputs(oracle, 0x89ABCDEF, 0x01234567, 0xFFFFFFFF), seed=4)
        assert st == 0, msg
    assert c.config.as_tuple()[0] == 3
    och = oracle.load_circuit(hr.rewrite_config(c.to_blob(), rate, hr.QUERIES[rate]))
    betas, gammas, alphas = ev.uniform_challenges(11)
    for name, w in [("witness", wires)] + [(n, m) for n, m in ev.wire_matrices(wires.shape) if n in ("edge", "const(p-1)")]:
        zs = oc.partial_products(w, betas, gammas)
        assert (och.partial_products(w, betas, gammas) == zs).all(), name
        q3 = oc.quotient(w, zs, betas, gammas, alphas)
        assert q3.any() and (och.quotient(w, zs, betas, gammas, alphas) == q3).all(), (name, rate)


def test_small_circuit_holds_every_inner_gate_kind(small):
    c, _oc, _wires = small
    assert set(stage_circuits.first_row_of_each_kind(c.to_blob())) == set(range(1, 11))


def test_oracle_zs_are_non_zero_for_every_stage_input_class(small):
    """The condition of the partial-product / quotient edge tests, on the reference alone: no denominator
    w + beta * sigma + gamma vanishes (inverting zero is outside the contract), i.e. every word of the oracle's zs_pp is
    non-zero -- for every wire class under uniform challenges, and for edge wires under every boundary challenge."""
    _c, oc, wires = small
    betas, gammas, alphas = ev.uniform_challenges(11)
    classes = [("witness", wires)] + list(ev.wire_matrices(wires.shape))
    for name, w in classes:
        zs = oc.partial_products(w, betas, gammas)
        assert zs.all(), name
        q = oc.quotient(w, zs, betas, gammas, alphas)
        assert (q < np.uint64(P)).all() and (zs < np.uint64(P)).all(), name
    edge_wires = dict(classes)["edge"]
    n_cases = 0
    for name, b, g, a in ev.boundary_challenge_cases():
        zs = oc.partial_products(edge_wires, b, g)
        assert zs.all(), name
        assert (oc.quotient(edge_wires, zs, b, g, a) < np.uint64(P)).all(), name
        n_cases += 1
    assert n_cases == 15
    # and the rule does exclude something: beta = gamma = 0 leaves w alone in the denominator, which is 0 somewhere
    zero = np.zeros(2, dtype=np.uint64)
    assert not oc.partial_products(edge_wires, zero, zero).all()
