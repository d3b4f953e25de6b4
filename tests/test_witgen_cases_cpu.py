"""No GPU: the circuits and operand tables of tests/witgen_cases.py meet their conditions on the reference alone.

Every circuit is accepted by the product's host importer and by the oracle; every row of every table has oracle status 0, the
oracle's witness equals the plain-Python model on every modelled wire, satisfies every gate and copy constraint
(`check_constraints`, the oracle's gate EVALUATORS, which share no code with its generators) and is canonical.  This is the
only place the oracle's `run_generator` meets a model that is not a restatement of the kernel's switch.
"""
import re

import numpy as np
import pytest

import blob_writer as bw
import witgen_cases as wc
from witgen_cases import P

PU = np.uint64(P)
# Gate::id() per blob gate kind, as INTEGRATION.md section 5 spells them (".." stands for parameters it leaves out)
GATE_IDS = {k: v[1] for k, v in bw.GATE_ORDER.items()}


@pytest.fixture(scope="module")
def cases():
    return wc.all_cases()


@pytest.fixture(scope="module")
def loaded(cases, oracle):
    return {name: oracle.load_circuit(c.blob) for name, c in cases.items()}


def _id_matches(product_id, spec_id):
    """`..` of the specification's text stands for anything; it also leaves out a trailing `<D=2>`."""
    parts = [re.escape(s) for s in spec_id.split("..")]
    return re.fullmatch(".*".join(parts) + r"(<D=2>)?", product_id) is not None


def test_names_cover_the_cases(cases):
    assert list(cases) == wc.NAMES and set(wc.FULL_BATCH) <= set(cases)


@pytest.mark.parametrize("name", wc.NAMES)
def test_circuit_is_accepted_by_the_host_importer_and_the_oracle(p25, cases, loaded, name):
    case = cases[name]
    circ = p25.Circuit.from_blob(case.blob)
    assert int(circ.info.degree_bits) <= 6
    assert int(circ.info.num_inputs) == case.n_ops + len(case.principal)
    ids = list(circ.gate_counts())
    kinds = case.gates | {bw.G_CONSTANT, bw.G_PUBLIC_INPUT}
    for k in kinds:
        assert sum(_id_matches(i, GATE_IDS[k]) for i in ids) == 1, (name, GATE_IDS[k], ids)
    for i in ids:                                       # and nothing else but padding
        assert any(_id_matches(i, GATE_IDS[k]) for k in kinds | {bw.G_NOOP}), (name, i)
    # the order of the gate table: (degree, id), upstream's
    assert ids == sorted(ids, key=lambda i: next((bw.GATE_ORDER[k][0], i) for k in bw.GATE_ORDER if _id_matches(i, GATE_IDS[k])))
    oc = loaded[name]
    assert oc.num_inputs == case.n_ops + len(case.principal) and oc.n == 1 << int(circ.info.degree_bits)
    assert p25.Circuit.from_blob(circ.to_blob()).info.num_generators == circ.info.num_generators


def test_constraint_counts_of_the_writer_are_the_evaluators(oracle):
    """blob_writer's num_constraints per gate kind against what the oracle's evaluators write (oracle/ref_gates.h)."""
    for kind, want in bw.GATE_CONSTRAINTS.items():
        out = oracle.eval_gate(kind, np.zeros((bw.NUM_WIRES, 2), dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64),
                               np.zeros(4, dtype=np.uint64))
        assert len(out) == want, (kind, len(out), want)


def test_every_generator_kind_is_in_some_circuit(cases):
    seen = {}
    for name, case in cases.items():
        kinds = {k for k, _d, _o in wc.generator_kinds(case.blob)}
        assert case.kinds <= kinds, (name, case.kinds - kinds)
        for k in kinds:
            seen.setdefault(k, name)
    assert sorted(seen) == list(range(21)), sorted(seen)


def test_mixed_circuit_has_both_permutations_in_the_first_level(cases):
    """Every dependency of the Poseidon2 generator and of the Poseidon generator is a circuit input (by the representative
    map), so both are ready before any generator has run: one level."""
    blob = cases["mixed_poseidon"].blob
    inputs, rep = wc.blob_tables(blob)
    input_reps = {rep[t] for t in inputs}
    perms = [(k, d) for k, d, _o in wc.generator_kinds(blob) if k in (bw.GEN_POSEIDON2, bw.GEN_POSEIDON)]
    assert sorted(k for k, _d in perms) == [bw.GEN_POSEIDON2, bw.GEN_POSEIDON]
    for k, deps in perms:
        assert len(deps) == 13 and all(rep[t] in input_reps for t in deps), k


def _check_row(case, oc, ops, what):
    wires, st, msg = oc.witness(case.inputs(ops), seed=5)
    assert st == 0, (what, st, msg)
    assert (wires < PU).all(), what
    model = case.wires(ops)
    assert model or case.name == "quotient_extension"           # its outputs are virtual targets: the expectations carry them
    for (row, col), v in model.items():
        assert int(wires[col][row]) == v, (what, "wire", row, col, hex(int(wires[col][row])), hex(v))
    bad, msg = oc.check_constraints(wires)
    assert bad == 0, (what, msg)


@pytest.mark.parametrize("name", wc.NAMES)
def test_oracle_witness_of_every_row_equals_the_model(cases, loaded, name):
    case = cases[name]
    for r, ops in enumerate(case.rows):
        _check_row(case, loaded[name], ops, (name, r, [hex(v) for v in ops][:8]))


@pytest.mark.parametrize("name", wc.NAMES)
def test_one_wrong_expectation_is_a_conflict(cases, loaded, name):
    case = cases[name]
    for which in (0, len(case.principal) - 1):
        assert loaded[name].witness(case.wrong(case.rows[len(case.rows) // 2], which), seed=5)[1] == 4, (name, which)


def test_u32_arithmetic_first_row_takes_the_zero_difference_branch(cases):
    low, high, inv, limbs = wc.u32_arithmetic_model(*wc.U32_TRIPLES[0])
    assert high == (1 << 32) - 1 and low == 0 and inv == 0
    assert all(wc.u32_arithmetic_model(*t)[2] != 0 for t in wc.U32_TRIPLES[1:])
    assert sorted(wc.u32_arithmetic_model(*wc.ALL_BUT_ONE_LIMB_3)[3]) == [2] + [3] * 31


def test_mixed_level_rows_with_a_non_boolean_swap(cases, loaded):
    """swap = 2 and swap = p - 1: the generators write delta = swap (b - a) and exchange nothing; the gate's swap (swap - 1)
    constraint does not hold, and nothing else is violated that the model does not predict."""
    case, oc = cases["mixed_poseidon"], loaded["mixed_poseidon"]
    for swap in (2, P - 1):
        for ops in wc.mixed_swap_rows(swap):
            wires, st, msg = oc.witness(case.inputs(ops), seed=5)
            assert st == 0, msg
            for (row, col), v in case.wires(ops).items():
                assert int(wires[col][row]) == v, (swap, row, col)
            assert oc.check_constraints(wires)[0] > 0


# ---- where upstream's generators panic -------------------------------------------------------------------------------------
def test_random_access_index_outside_the_list_is_status_7_on_the_oracle(cases, loaded):
    """The oracle's generator throws; p25o_witness and p25o_prove answer 7 (P25_ERR_INTERNAL, the kernel's code) with the
    message and leave the process alive."""
    case, oc = cases["random_access"], loaded["random_access"]
    for index in (16, P - 1):
        inp = case.inputs(case.rows[3])
        inp[:case.n_ops] = wc.random_access_bad_index_row(case, index)
        _w, st, msg = oc.witness(inp, seed=5)
        assert st == 7 and "index" in msg, (index, st, msg)
        assert oc.prove(inp, seed=5)[1] == 7
        assert oc.witness_forced(inp, seed=5)[1] == 7


def test_zero_divisors_on_the_oracle(cases, loaded):
    """inv(0) = 0 in the oracle as on the device (include/p25.h): a zero denominator gives the quotient 0, which the
    circuit's q den == num refuses unless num is 0 too; a zero shift gives the shifted point 0 and status 0 with a witness
    that violates the gate's point == x shift."""
    case, oc = cases["quotient_extension"], loaded["quotient_extension"]
    assert oc.witness(case.inputs(wc.QUOTIENT_ZERO_DIVISOR["num != 0"]), seed=5)[1] == 4
    wires, st, _m = oc.witness(case.inputs(wc.QUOTIENT_ZERO_DIVISOR["num == 0"]), seed=5)
    assert st == 0 and oc.check_constraints(wires)[0] == 0
    case, oc = cases["coset_interpolation"], loaded["coset_interpolation"]
    ops = wc.coset_zero_shift_row(case)
    assert ops[33] or ops[34]
    wires, st, msg = oc.witness(case.inputs(ops), seed=5)
    assert st == 0, msg
    for (row, col), v in case.wires(ops).items():
        assert int(wires[col][row]) == v, (row, col)
    assert int(wires[45][0]) == 0 and int(wires[46][0]) == 0
    assert oc.check_constraints(wires)[0] > 0
