"""CPU: the oracle's forging prover (oracle/ref_prover.h RFault) and the fault table of tests/forged_proofs.py, on the
`and` gadget (2^4 rows, no FRI layer) and its recursive verifier (2^11 rows, two FRI layers).

What is checked here is the test infrastructure itself: that no fault is a second prover (kind 0 is prove() word for
word, and a fault leaves alone every word of the proof that is written ahead of it), that the oracle's verifier answers
each forged proof with the code the table writes down, and that a fault the circuit has no place for is refused and
never answered with an honest proof."""
import numpy as np
import pytest

import forged_proofs as fp
from conftest import P
from verify_cases import CAP_WORDS, Layout, expected


class Host:
    def __init__(self, oracle, c, inputs, seed):
        self.c, self.oc, self.inputs, self.seed = c, oracle.load_circuit(c.to_blob()), np.asarray(inputs, dtype=np.uint64), seed
        self.proof, st, _t, msg = self.oc.prove(self.inputs, seed=seed)
        assert st == 0, msg
        self.dg, self.cap = self.oc.digest()
        self.L = Layout(c)
        self.forged = fp.forge(self.oc, c, self.inputs)

    def named(self, name):
        return next(f for f in self.forged if f.name == name)


@pytest.fixture(scope="module")
def flat(p25, oracle):
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    return Host(oracle, p25.Circuit.build_gadget(0, 0), [x, y, (x & y) % P], fp.SEEDS["flat"])


@pytest.fixture(scope="module")
def layers(p25, oracle, flat):
    outer = flat.c.build_recursive_verifier(1, flat.dg, flat.cap)
    host = Host(oracle, outer, flat.proof, fp.SEEDS["layers"])
    assert int(outer.info.degree_bits) == 11 and host.L.n_layers == 2 and int(outer.info.proof_words) == 15189
    return host


@pytest.fixture(scope="module", params=["flat", "layers"])
def host(request):
    return request.getfixturevalue(request.param)


def test_no_fault_is_the_honest_prover_word_for_word(host):
    proof, st, msg = host.oc.prove_forged(host.inputs, host.seed, (fp.NONE, 0, 0))
    assert st == 0, msg
    assert (proof == host.proof).all()
    assert expected(host.oc, proof, host.dg, host.cap) == 0


def test_the_oracle_answers_every_forged_proof_with_the_tables_code(host):
    shape = fp.shape_of(host.c)
    assert [f.name for f in host.forged] == [r.name for r in fp.TABLE if getattr(r, shape) is not None]
    got = fp.oracle_codes(host.oc, host.forged, host.dg, host.cap)
    assert got == [f.code for f in host.forged], [(f.name, g, f.code) for f, g in zip(host.forged, got) if g != f.code]
    assert set(got) == ({fp.VANISHING, fp.FRI_EVAL, fp.FINAL_POLY} if shape == "layers" else {fp.VANISHING, fp.FINAL_POLY})


def test_a_fault_changes_nothing_that_is_written_ahead_of_it(host):
    """The proof sections in the order the prover fixes them: wires cap | zs cap, quotient cap | openings | FRI caps in
    turn | final polynomial (the query rounds follow the PoW and move with any change)."""
    L, honest = host.L, host.proof
    same = lambda f, end: (f.proof[:end] == honest[:end]).all()   # noqa: E731
    assert not same(host.named("wire"), CAP_WORDS)
    for f in host.forged:
        if f.kind == fp.OPENING:
            assert same(f, L.constants) and not same(f, L.openings_end), f.name
            changed = np.nonzero(f.proof[L.constants:L.openings_end] != honest[L.constants:L.openings_end])[0] // 2
            Q = int(host.c.info.quotient_degree_factor)
            solved = {fp.opening_index(host.c, "quotient", 1) - 1 + Q * i for i in range(int(host.c.info.num_challenges))}
            assert f.fault[1] in changed and set(changed.tolist()) <= {f.fault[1]} | solved, f.name
        if f.kind == fp.FRI_LAYER:
            end = L.fri_caps + CAP_WORDS * f.fault[1]
            assert same(f, end) and not same(f, end + CAP_WORDS), f.name
        if f.kind == fp.FRI_FOLD:
            end = L.fri_caps + CAP_WORDS * (f.fault[1] + 1)                  # the folded layer itself is committed honestly
            assert same(f, end), f.name
        if f.kind == fp.FINAL:
            assert same(f, L.queries), f.name
            k = 2 * f.fault[1] + f.fault[2]
            diff = (f.proof[L.final_poly:L.pow_witness].astype(object) - honest[L.final_poly:L.pow_witness].astype(object)) % P
            assert diff.tolist() == [int(j == k) for j in range(2 * L.final_poly_len)], f.name


def test_faults_without_a_place_are_refused_not_proved_honestly(host):
    i = host.c.info
    n_openings = sum(fp.section_sizes(host.c).values())
    solved = fp.opening_index(host.c, "quotient", 1) - 1
    bad = [(fp.OPENING, n_openings, 0), (fp.OPENING, 1 << 40, 0), (fp.OPENING, solved, 0),
           (fp.OPENING, solved + int(i.quotient_degree_factor), 0), (fp.WIRE, int(i.num_wires), 0), (fp.WIRE, 0, 1 << int(i.degree_bits)),
           (fp.FRI_LAYER, host.L.n_layers, 0), (fp.FRI_FOLD, host.L.n_layers, 0), (fp.FRI_LAYER, 0, 2),
           (fp.FINAL, host.L.final_poly_len, 0), (fp.FINAL, 0, 2), (6, 0, 0), (-1, 0, 0)]
    for fault in bad:
        proof, st, msg = host.oc.prove_forged(host.inputs, host.seed, fault)
        assert st == fp.REFUSED and msg.startswith("fault:") and not proof.any(), (fault, st, msg)
    # the last opening and the last wire are still in range
    for fault in ((fp.OPENING, n_openings - 1, 0), (fp.WIRE, int(i.num_wires) - 1, (1 << int(i.degree_bits)) - 1)):
        assert host.oc.prove_forged(host.inputs, host.seed, fault)[1] == 0, fault
