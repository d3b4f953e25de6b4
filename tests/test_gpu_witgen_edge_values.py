"""GPU: the device witness generators (kernels_witgen.hip, blob kinds 0 to 20) on boundary operands, kind by kind.

The circuits, operand tables and plain-Python models are tests/witgen_cases.py's; tests/test_witgen_cases_cpu.py shows on the
CPU that every row has oracle status 0 and that the oracle's witness is the model's.  Here the device meets both: wire for
wire (`p25_witness`), in batches on either side of the witness pass size (`p25_prove_batch`: the per-lane index split and the
cooperative group clamp with a partially filled last block), with a Poseidon2 and a Poseidon generator in one level (the
per-lane `case GEN_POSEIDON` body), with failures in the middle of a batch, and where upstream's generators panic.

Every comparison is equality; every word is asserted canonical.
"""
import os
import re

import numpy as np
import pytest

import witgen_cases as wc
from conftest import ROOT
from witgen_cases import P

pytestmark = pytest.mark.gpu
PU = np.uint64(P)
P25_ERR_WITNESS_CONFLICT, P25_ERR_INTERNAL = 4, 7


def witness_pass_size():
    """Proofs per witness pass: `MAXB` of DeviceCircuit::prove_batch_dev (the 64 of launch_witgen's comment)."""
    src = open(os.path.join(ROOT, "plonky2.5_amd", "csrc", "prover.hip")).read()
    return int(re.search(r"const size_t MAXB = (\d+);", src).group(1))


@pytest.fixture(scope="module")
def cases():
    return wc.all_cases()


@pytest.fixture(scope="module")
def circuits(gpu, oracle, cases):
    """name -> (device circuit, oracle circuit), each built once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (gpu.Circuit.from_blob(cases[name].blob), oracle.load_circuit(cases[name].blob))
        return made[name]

    return get


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got < PU).all(), (what, "non-canonical word at", np.argwhere(got >= PU)[:5].tolist())
    diff = np.argwhere(got != want)
    assert diff.size == 0, (what, "first differing words", diff[:5].tolist(), len(diff), "of", got.size)


def _model_wires(case, wires, ops, what):
    for (row, col), v in case.wires(ops).items():
        assert int(wires[col][row]) == v, (what, "wire", row, col, hex(int(wires[col][row])), "model", hex(v))


# ---- a. wire for wire -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_witness_of_every_row_equals_the_oracles_and_the_model(cases, circuits, name):
    case = cases[name]
    c, oc = circuits(name)
    for r, ops in enumerate(case.rows):
        what = (name, r, [hex(v) for v in ops][:8])
        inp = case.inputs(ops)
        wg, st = c.witness(inp, seed=100 + r)
        wo, sto, msg = oc.witness(inp, seed=100 + r)
        assert st == 0 and sto == 0, (what, st, sto, msg)
        _same(wg, wo, what)
        _model_wires(case, wg, ops, what)
        bad, msg = oc.check_constraints(wg)
        assert bad == 0, (what, msg)


def test_u32_arithmetic_zero_difference_branch(cases, circuits):
    """x = y = z = 2^32 - 1: x y + z = p - 1, high = 2^32 - 1, low = 0, and the inverse wire holds 0 (diff == 0 ? 0 : inv)."""
    case = cases["u32_arithmetic"]
    c, _oc = circuits("u32_arithmetic")
    ops = case.rows[0]
    assert ops[:3] == [(1 << 32) - 1] * 3
    low, high, inv, _limbs = wc.u32_arithmetic_model(*ops[:3])
    assert high == (1 << 32) - 1 and low == 0 and inv == 0
    wires, st = c.witness(case.inputs(ops), seed=1)
    assert st == 0 and [int(wires[k][0]) for k in (3, 4, 5)] == [low, high, inv]


# ---- b. the batch forms -------------------------------------------------------------------------------------------------------
def _prove_batch(case, c, oc, n, what, dg_cap):
    """n proofs, the table's rows in turn: statuses 0, the device verifier accepts all, and the proofs at `spots` are the
    oracle's words and pass its verifier."""
    maxb = witness_pass_size()
    rows = [case.rows[i % len(case.rows)] for i in range(n)]
    batch = np.stack([case.inputs(ops) for ops in rows])
    seeds = [7 + i for i in range(n)]
    proofs, st = c.prove(batch, seeds=seeds)
    assert st.tolist() == [0] * n, (what, n, np.argwhere(st != 0)[:5].tolist(), st[st != 0][:5].tolist())
    assert (proofs < PU).all(), (what, n)
    assert c.verify(proofs).tolist() == [0] * n, (what, n)
    spots = sorted({i for i in (0, n - 1, maxb - 1, maxb) if 0 <= i < n})
    for i in spots:
        po, sto, _t, msg = oc.prove(batch[i], seed=seeds[i])
        assert sto == 0, (what, n, i, msg)
        _same(proofs[i], po, (what, "batch of", n, "proof", i))
        assert oc.verify(proofs[i], *dg_cap)[0] == 0, (what, n, i)


@pytest.mark.parametrize("name", wc.NAMES)
def test_all_rows_in_one_batch(cases, circuits, name):
    c, oc = circuits(name)
    _prove_batch(cases[name], c, oc, len(cases[name].rows), name, c.digest())


def test_witness_pass_size_is_the_one_the_batch_sizes_straddle():
    assert witness_pass_size() == 64


@pytest.mark.parametrize("n_off", [(1, 0), (2, 0), (17, 0), (0, -1), (0, 0), (0, 1)], ids=["1", "2", "17", "pass-1", "pass", "pass+1"])
@pytest.mark.parametrize("name", wc.FULL_BATCH)
def test_batch_sizes_around_the_witness_pass(cases, circuits, name, n_off):
    """A partially filled last block under the per-lane split (idx / n_proofs, idx % n_proofs) and under the cooperative
    group clamp (!valid): with one permutation a proof a block holds 16 groups, so 1, 2 and 17 proofs and the one proof of
    the second pass at pass + 1 all leave lanes over."""
    n = n_off[0] or witness_pass_size() + n_off[1]
    c, oc = circuits(name)
    _prove_batch(cases[name], c, oc, n, name, c.digest())


# ---- c. the mixed level ---------------------------------------------------------------------------------------------------------
def test_mixed_level_swaps_on_either_kind(cases, circuits):
    """swap 0 / 1 on the Poseidon2 row and on the Poseidon row, all four combinations present in the table (whose rows tests a
    and b run): here the per-lane Poseidon row is checked against the model on its own, exchange and no exchange."""
    case = cases["mixed_poseidon"]
    c, oc = circuits("mixed_poseidon")
    combos = {(ops[12], ops[25]) for ops in case.rows}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    p_row = max(t[1] for t in case.principal)
    for r, ops in enumerate(case.rows):
        wg, st = c.witness(case.inputs(ops), seed=r)
        assert st == 0
        st_in, swap = ops[13:25], ops[25]
        tr, out = wc.poseidon_trace(st_in[4:8] + st_in[0:4] + st_in[8:12] if swap == 1 else st_in)
        assert [int(wg[12 + i][p_row]) for i in range(12)] == out, (r, swap)
        assert [int(wg[29 + i][p_row]) for i in range(106)] == tr, (r, swap)


@pytest.mark.parametrize("swap", [2, P - 1], ids=["2", "p-1"])
def test_mixed_level_non_boolean_swap(cases, circuits, swap):
    """The generators are defined for any swap word: delta = swap (b - a), the halves exchanged for swap == 1 only.  The
    wires are the oracle's and the model's; the gate's swap (swap - 1) == 0 does not hold."""
    case = cases["mixed_poseidon"]
    c, oc = circuits("mixed_poseidon")
    for ops in wc.mixed_swap_rows(swap):
        inp = case.inputs(ops)
        wg, st = c.witness(inp, seed=3)
        wo, sto, msg = oc.witness(inp, seed=3)
        assert st == 0 and sto == 0, msg
        _same(wg, wo, ("mixed", swap))
        _model_wires(case, wg, ops, ("mixed", swap))
        assert oc.check_constraints(wg)[0] > 0


# ---- d. failures stay in their proof ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.NAMES)
def test_a_wrong_expectation_fails_its_own_proof_only(cases, circuits, name):
    case = cases[name]
    c, oc = circuits(name)
    a, b = case.rows[0], case.rows[-1]
    mid = case.rows[len(case.rows) // 2]
    good = np.stack([case.inputs(a), case.inputs(mid), case.inputs(b)])
    clean, st = c.prove(good, seeds=[1, 2, 3])
    assert st.tolist() == [0, 0, 0]
    bad = good.copy()
    bad[1] = case.wrong(mid, len(case.principal) - 1)
    proofs, st = c.prove(bad, seeds=[1, 2, 3])
    assert st.tolist() == [0, P25_ERR_WITNESS_CONFLICT, 0], st.tolist()
    _same(proofs[0], clean[0], (name, "proof before the failed one"))
    _same(proofs[2], clean[2], (name, "proof behind the failed one"))
    po, sto, _t, msg = oc.prove(good[2], seed=3)
    assert sto == 0, msg
    _same(proofs[2], po, (name, "proof behind the failed one, oracle"))


@pytest.mark.parametrize("index", [16, P - 1], ids=["16", "p-1"])
def test_random_access_index_outside_the_list(cases, circuits, index):
    """The kernel sets P25_ERR_INTERNAL for that proof (upstream: out-of-bounds panic); the oracle's generator throws and its
    witness and prover answer non-zero; the neighbours' proofs are the oracle's."""
    case = cases["random_access"]
    c, oc = circuits("random_access")
    batch = np.stack([case.inputs(case.rows[r]) for r in (2, 3, 4)])
    batch[1, :case.n_ops] = wc.random_access_bad_index_row(case, index)
    proofs, st = c.prove(batch, seeds=[1, 2, 3])
    assert st.tolist() == [0, P25_ERR_INTERNAL, 0], st.tolist()
    assert c.witness(batch[1], seed=2)[1] == P25_ERR_INTERNAL
    _w, sto, msg = oc.witness(batch[1], seed=2)
    assert sto != 0 and "index" in msg, (sto, msg)
    assert oc.prove(batch[1], seed=2)[1] != 0
    for i in (0, 2):
        po, sto, _t, msg = oc.prove(batch[i], seed=1 + i)
        assert sto == 0, msg
        _same(proofs[i], po, ("random access, neighbour", i))


# ---- e. zero divisors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(wc.QUOTIENT_ZERO_DIVISOR))
def test_quotient_extension_by_zero(cases, circuits, which):
    """include/p25.h: the inverse of zero is zero.  den = (0, 0) gives q = (0, 0); the circuit's q den == num then is a
    conflict for num != 0 (never P25_OK with a violated constraint) and a satisfied witness for num == 0."""
    case = cases["quotient_extension"]
    c, oc = circuits("quotient_extension")
    inp = case.inputs(wc.QUOTIENT_ZERO_DIVISOR[which])
    wg, st = c.witness(inp, seed=9)
    wo, sto, msg = oc.witness_forced(inp, seed=9)
    assert st == sto == (P25_ERR_WITNESS_CONFLICT if which == "num != 0" else 0), (st, sto, msg)
    _same(wg, wo, ("quotient by zero", which))
    assert (oc.check_constraints(wg)[0] == 0) == (st == 0)
    assert c.prove(inp, seeds=[9])[1].tolist() == [st]


def test_coset_interpolation_with_shift_zero(cases, circuits):
    """include/p25.h: shift = 0 gives the shifted point x = point inv(0) = 0 and the interpolant's value there; the status is
    0 on the device as on the oracle although the gate's point == x shift does not hold (the caller's error, upstream
    panics): the words are pinned, equal on both sides and the model's."""
    case = cases["coset_interpolation"]
    c, oc = circuits("coset_interpolation")
    ops = wc.coset_zero_shift_row(case)
    inp = case.inputs(ops)
    wg, st = c.witness(inp, seed=9)
    wo, sto, msg = oc.witness(inp, seed=9)
    assert st == sto == 0, (st, sto, msg)
    _same(wg, wo, "shift = 0")
    _model_wires(case, wg, ops, "shift = 0")
    assert int(wg[45][0]) == 0 and int(wg[46][0]) == 0 and oc.check_constraints(wg)[0] > 0
    # the proof made of that witness: status 0 from both provers, the same words, and no verifier takes it
    proofs, stp = c.prove(inp, seeds=[9])
    po, sto, _t, msg = oc.prove(inp, seed=9)
    assert stp.tolist() == [0] and sto == 0, (stp.tolist(), sto, msg)
    _same(proofs[0], po, "proof of the shift = 0 witness")
    assert c.verify(proofs)[0] != 0 and oc.verify(proofs[0], *c.digest())[0] != 0
