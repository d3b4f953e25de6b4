"""CPU: public values of the inner STARK (include/p25.h, "PUBLIC VALUES") -- the AIR form, the host prover, the
verifier-circuit builder.

An AIR declares n_public values and reads them with node op 6 PUBLIC; a proof's values are the last n_public words of its
flat input, observed by the challenger behind the trace commitment.  Expected verdicts come from the independent model
tests/p3_public_values_model.py; the outer circuit is judged by the oracle, loaded from the exported blob."""
import ctypes as C

import numpy as np
import pytest

import air_cases
import air_cases_pv
import p3_public_values_model as M
from conftest import P

OK, INVALID_ARG = 0, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _last(p25):
    return p25.lib().p25_last_error().decode()


def _create(p25, air, log_n=3, log_blowup=1, queries=3, pow_bits=4):
    ac, h = air.to_c(), C.c_void_p()
    st = p25.lib().p25_p3_prover_create(C.byref(ac), log_n, log_blowup, queries, pow_bits, C.byref(h))
    return st, h


# ---- 1. validation -------------------------------------------------------------------------------------------------
def test_public_index_and_count_are_validated(p25):
    air = air_cases_pv.fib_pv(p25)
    st, h = _create(p25, air)
    assert st == OK, _last(p25)
    p25.lib().p25_p3_prover_destroy(h)

    bad = p25.Air(3, n_public=3)
    bad.assert_zero(bad.sub(bad.local(0), bad.public(3)))               # index = n_public
    assert _create(p25, bad)[0] == INVALID_ARG and "public" in _last(p25)

    none = p25.Air(3)                                                   # a PUBLIC node at n_public = 0
    none.assert_zero(none.sub(none.local(0), none.public(0)))
    assert _create(p25, none)[0] == INVALID_ARG and "public" in _last(p25)

    many = p25.Air(3, n_public=65)
    many.assert_zero(many.sub(many.local(0), many.public(0)))
    assert _create(p25, many)[0] == INVALID_ARG and "public" in _last(p25)
    cap = p25.Air(3, n_public=64)
    cap.when_first_row(cap.sub(cap.local(0), cap.public(63)))
    st, h = _create(p25, cap)
    assert st == OK, _last(p25)
    p25.lib().p25_p3_prover_destroy(h)

    # the same refusals from the host prover and the circuit builder
    tr = air_cases.fib_trace(3)
    for a in (bad, none, many):
        with pytest.raises(p25.P25Error) as ei:
            p25.p3_prove_air(a, tr, num_queries=3, pow_bits=4, public_values=np.zeros(a.n_public, dtype=np.uint64))
        assert ei.value.status == INVALID_ARG
        with pytest.raises(p25.P25Error):
            p25.Circuit.build_p3_verifier_air(p25.P3Config(1, 3, 4, 0, 3, 3, 4, 2, 3), a)


def test_public_is_a_degree_zero_leaf(p25):
    """PUBLIC counts like CONST in the degree pass: public * local^2 under a selector is degree 3 (two chunks), not 4."""
    air = p25.Air(2, n_public=1)
    x = air.local(0)
    air.when_transition(air.sub(air.mul(air.public(0), air.mul(x, x)), air.next(1)))
    pr = p25.P3Prover(air, 3, 1, 3, 4)
    assert pr.config.log_quotient_degree == 1
    # a long chain of squarings is refused for its degree, whatever an int would make of 2^70
    deep = p25.Air(2)
    y = deep.local(0)
    for _ in range(70):
        y = deep.mul(y, y)
    deep.assert_zero(deep.sub(y, deep.local(1)))
    assert _create(p25, deep)[0] == INVALID_ARG and "degree" in _last(p25)


def test_the_forms_without_public_values_refuse_such_an_air(p25):
    lib = p25.lib()
    air = air_cases_pv.fib_pv(p25)
    tr, pv = air_cases_pv.fib_pv_trace(3, 2, 3)
    ac, n = air.to_c(), C.c_size_t(0)
    out = np.zeros(4096, dtype=np.uint64)
    st = lib.p25_p3_prove_air(C.byref(ac), _p(tr), 3, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pv" in _last(p25)
    st = lib.p25_p3_prove_air_ex(C.byref(ac), _p(tr), 3, 1, 3, 4, 0, 1, _p(out), out.size, C.byref(n), None)
    assert st == INVALID_ARG and "p25_p3_prove_air_pv" in _last(p25)

    # p25_p3_prover_create itself accepts it; num_inputs = the proof's words + n_public
    pr = p25.P3Prover(air, 3, 1, 3, 4)
    assert pr.n_public == 3
    assert pr.num_inputs == M.Shape(pr.config).num_inputs + 3
    plain = p25.P3Prover(p25.Air.fibonacci(), 3, 1, 3, 4)
    assert plain.n_public == 0 and pr.num_inputs == plain.num_inputs + 3
    assert bytes(pr.config) == bytes(plain.config)                      # p25_p3_config does not change
    status = np.zeros(1, dtype=np.int32)
    rows = np.zeros((1, pr.num_inputs), dtype=np.uint64)
    st = lib.p25_p3_prove_batch(pr._h, _p(tr), 1, None, _p(rows), pr.num_inputs, _p(status))
    assert st == INVALID_ARG and "p25_p3_prove_batch_pv" in _last(p25)
    # the device form is refused on its arguments, before any device is looked for (the pointers are never followed)
    st = lib.p25_p3_prove_batch_dev(pr._h, _p(tr), tr.size, 1, None, _p(rows), pr.num_inputs, _p(status), None)
    assert st == INVALID_ARG and "p25_p3_prove_batch_pv_dev" in _last(p25)
    # the host _pv form checks every public value < p before anything is launched
    big = pv.copy()
    big[1] = P
    st = lib.p25_p3_prove_batch_pv(pr._h, _p(tr), _p(big), 1, None, _p(rows), pr.num_inputs, _p(status))
    assert st == INVALID_ARG and "public_values" in _last(p25)
    st = lib.p25_p3_prove_batch_pv(pr._h, _p(tr), None, 1, None, _p(rows), pr.num_inputs, _p(status))
    assert st == INVALID_ARG
    st = lib.p25_p3_prove_batch_pv(pr._h, _p(tr), _p(pv), 1, None, _p(rows), pr.num_inputs - 1, _p(status))
    assert st == INVALID_ARG and "stride" in _last(p25)                 # the stride counts the tail
    assert not rows.any()


# ---- 2. host prover ------------------------------------------------------------------------------------------------
def _check_proof(p25, oracle, air, trace, pv, queries, pow_bits, log_blowup):
    inp, cfg = p25.p3_prove_air(air, trace, num_queries=queries, pow_bits=pow_bits, log_blowup=log_blowup, threads=1,
                                public_values=pv)
    m = air.n_public
    assert inp.size == M.Shape(cfg).num_inputs + m
    assert (inp[inp.size - m:] == np.asarray(pv, dtype=np.uint64)).all()
    assert M.verify(oracle, air, cfg, inp) == M.OK
    for i in sorted({0, m // 2, m - 1}):                                # one tail word changed: the model rejects
        t = inp.copy()
        t[inp.size - m + i] = (int(t[inp.size - m + i]) + 1) % P
        assert M.verify(oracle, air, cfg, t) != M.OK, i
    return inp, cfg


@pytest.mark.parametrize("log_n,log_blowup", [(3, 1), (3, 2), (6, 1), (6, 2)])
def test_host_prover_fib_pv(p25, oracle, log_n, log_blowup):
    air = air_cases_pv.fib_pv(p25)
    trace, pv = air_cases_pv.fib_pv_trace(log_n, 3 + log_n, 1 << 40)
    inp, cfg = _check_proof(p25, oracle, air, trace, pv, 3, 4, log_blowup)
    # the values are part of the transcript: other first-row values, another proof from its first sampled word on
    trace2, pv2 = air_cases_pv.fib_pv_trace(log_n, 4 + log_n, 1 << 40)
    inp2, _ = p25.p3_prove_air(air, trace2, num_queries=3, pow_bits=4, log_blowup=log_blowup, threads=1, public_values=pv2)
    assert (inp2[:4] != inp[:4]).any() and M.verify(oracle, air, cfg, inp2) == M.OK
    # a trace whose last row disagrees with pv2
    wrong = pv.copy()
    wrong[2] = (int(wrong[2]) + 1) % P
    with pytest.raises(p25.P25Error) as ei:
        p25.p3_prove_air(air, trace, num_queries=3, pow_bits=4, log_blowup=log_blowup, threads=1, public_values=wrong)
    assert ei.value.status == INVALID_ARG
    big = pv.copy()
    big[0] = P
    with pytest.raises(p25.P25Error) as ei:
        p25.p3_prove_air(air, trace, num_queries=3, pow_bits=4, log_blowup=log_blowup, threads=1, public_values=big)
    assert ei.value.status == INVALID_ARG


@pytest.mark.parametrize("m", [1, 4, 5, 13])
def test_host_prover_pv_mix(p25, oracle, m):
    air = air_cases_pv.pv_mix(p25, m)
    pv = air_cases_pv.pv_mix_values(m, 0)
    _check_proof(p25, oracle, air, air_cases_pv.pv_mix_trace(3, pv), pv, 2, 3, 1)
    # every public value enters under its own weight: two of them swapped no longer fit the trace
    if m > 1:
        swapped = pv.copy()
        swapped[[0, m - 2]] = swapped[[m - 2, 0]]
        assert int(pv[0]) != int(pv[m - 2])
        with pytest.raises(p25.P25Error):
            p25.p3_prove_air(air, air_cases_pv.pv_mix_trace(3, pv), num_queries=2, pow_bits=3, public_values=swapped)


def test_pv_form_without_public_values_gives_the_plain_words(p25):
    air, trace = p25.Air.fibonacci(), air_cases.fib_trace(4)
    want, cfg = p25.p3_prove_air(air, trace, num_queries=4, pow_bits=5, log_blowup=2, threads=1)
    ac, n, c2 = air.to_c(), C.c_size_t(0), p25.P3Config()
    lib = p25.lib()
    assert lib.p25_p3_prove_air_pv(C.byref(ac), _p(trace), None, 4, 2, 4, 5, 0, 1, None, 0, C.byref(n), C.byref(c2)) == OK
    assert n.value == want.size                                         # the size query
    out = np.zeros(n.value, dtype=np.uint64)
    assert lib.p25_p3_prove_air_pv(C.byref(ac), _p(trace), None, 4, 2, 4, 5, 0, 1, _p(out), out.size, C.byref(n), C.byref(c2)) == OK
    assert (out == want).all() and bytes(c2) == bytes(cfg)
    # and the size query of an AIR with public values counts them
    air3 = air_cases_pv.fib_pv(p25)
    ac3 = air3.to_c()
    assert lib.p25_p3_prove_air_pv(C.byref(ac3), None, None, 4, 2, 4, 5, 0, 1, None, 0, C.byref(n), None) == OK
    assert n.value == want.size + 3


def test_json_forms_cover_the_proof_words_only(p25):
    air = air_cases_pv.fib_pv(p25)
    trace, pv = air_cases_pv.fib_pv_trace(3, 7, 8)
    inp, cfg = p25.p3_prove_air(air, trace, num_queries=3, pow_bits=4, public_values=pv)
    js = p25.p3_inputs_to_json(inp[:inp.size - 3], cfg)
    back, cfg2 = p25.p3_proof_from_json(js)
    assert (back == inp[:inp.size - 3]).all()
    assert (cfg2.trace_width, cfg2.log_trace_height, cfg2.num_queries) == (3, 3, 3)
    with pytest.raises(p25.P25Error):
        p25.p3_inputs_to_json(inp, cfg)


# ---- 3. the verifier circuit ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fib_pv_outer(p25, oracle):
    air = air_cases_pv.fib_pv(p25)
    trace, pv = air_cases_pv.fib_pv_trace(3, 5, 9)
    inp, cfg = p25.p3_prove_air(air, trace, num_queries=3, pow_bits=4, threads=1, public_values=pv)
    c = p25.Circuit.build_p3_verifier_air(cfg, air)
    return air, cfg, inp, pv, c, oracle.load_circuit(c.to_blob())


def test_circuit_registers_the_public_values(p25, fib_pv_outer):
    air, cfg, inp, pv, c, oc = fib_pv_outer
    assert int(c.info.num_public_inputs) == 3
    assert int(c.info.num_inputs) == M.Shape(cfg).num_inputs + 3 == inp.size
    plain = p25.Circuit.build_p3_verifier_air(cfg, p25.Air.fibonacci())
    assert int(plain.info.num_public_inputs) == 0 and int(plain.info.num_inputs) == inp.size - 3
    assert plain.to_blob() == p25.Circuit.build_p3_verifier(cfg).to_blob()      # n_public = 0: the circuit as it was


def test_oracle_proves_and_verifies_the_outer_circuit(fib_pv_outer):
    air, cfg, inp, pv, c, oc = fib_pv_outer
    wires, st, msg = oc.witness(inp, seed=3)
    assert st == 0, msg
    bad, msg = oc.check_constraints(wires)
    assert bad == 0, msg
    proof, st, _tm, msg = oc.prove(inp, seed=3)
    assert st == 0, msg
    assert proof[-3:].tolist() == [int(v) for v in pv] == [5, 9, int(pv[2])]
    assert oc.verify(proof)[0] == 0
    claimed = proof.copy()                                              # the proof does not carry other public inputs
    claimed[-1] = (int(claimed[-1]) + 1) % P
    assert oc.verify(claimed)[0] != 0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_changed_tail_word_is_a_witness_conflict(fib_pv_outer, which):
    air, cfg, inp, pv, c, oc = fib_pv_outer
    t = inp.copy()
    t[inp.size - 3 + which] = (int(t[inp.size - 3 + which]) + 1) % P
    assert oc.witness(t, seed=3)[1] == 4                                # P25_ERR_WITNESS_CONFLICT
