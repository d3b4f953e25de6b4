"""Forged proofs that fail exactly one check of the plonky2 verifier: the fault table and the helper that forges it.

A flipped word of a finished proof moves the Fiat-Shamir transcript, so it is rejected by the vanishing identity, the PoW
or an initial Merkle path whatever check the word belongs to.  The oracle's forging prover (oracle/ref_prover.h RFault)
tampers with one value at one point of the proof and finishes the proof honestly on the tampered data, so that the
proof fails the targeted check and nothing ahead of it.  Shared by tests/test_forged_proofs_cpu.py (the oracle's own
verifier), test_verify_lanes_cpu.py (the lanes on the host), test_recursion_cpu.py (the in-circuit verifier) and
test_gpu_forged_proofs.py (the kernels and the device witness generator).

The codes below are written down from the verifier's documented order of checks (include/p25.h), never read from a
verifier.  Two circuit shapes: "layers" = FRI reduction layers 0 and 1 (the 2^11-row recursive verifier of the `and`
gadget), "flat" = none (the `and` gadget itself, 2^4 rows: the batched polynomial is the final polynomial).  None = the
shape has no place for the fault and the forging prover must refuse it with status 1.

  WIRE       the constraints no longer vanish on the subgroup, the quotient is no polynomial of its degree      -> VANISHING
  OPENING    the identity at zeta is made to hold; (p(X) - opening) / (X - zeta) is what the verifier folds from, and
             it is not the committed batched polynomial: the first comparison of a query sees it      -> FRI_EVAL / FINAL_POLY
  FRI_LAYER  a committed layer that is not the fold of the one before it: the layer's own comparison fails.  Mask 1
             bumps the even slots of every leaf only: a query whose index at that layer is even fails there, an odd one
             passes and fails the NEXT comparison, because its fold read a bumped neighbour.  At layer 0 both ends are
             FRI_EVAL; at the last layer the odd case is FINAL_POLY, so FRI_EVAL there is a property of query 0's index,
             hence of the seed: the tests assert it from the oracle's verdict                                   -> FRI_EVAL
  FRI_FOLD   layer l+1 (or the final polynomial) is an honest commitment to a wrong fold          -> FRI_EVAL / FINAL_POLY
  FINAL_POLY                                                                                                   -> FINAL_POLY
"""
from collections import namedtuple

import numpy as np

from verify_cases import FINAL_POLY, FRI_EVAL, VANISHING, Layout, expected

NONE, WIRE, OPENING, FRI_LAYER, FRI_FOLD, FINAL = range(6)
REFUSED = 1                                  # the forging prover's status for a fault the circuit has no place for

# An opening is named by its section and its element there; `opening_index` turns that into the prover's index.
SECTIONS = ("constants", "sigmas", "wires", "zs", "zs_next", "pps", "quotient")
Row = namedtuple("Row", "name kind a b layers flat")
TABLE = (
    Row("wire",                 WIRE,      0, 0,              VANISHING,  VANISHING),      # column 0, row 0: routed and read by its gate
    Row("opening_constant",     OPENING,   ("constants", 0),  0, FRI_EVAL, FINAL_POLY),
    Row("opening_sigma",        OPENING,   ("sigmas", 7),     0, FRI_EVAL, FINAL_POLY),
    Row("opening_wire_unread",  OPENING,   ("wires", -1),     0, FRI_EVAL, FINAL_POLY),   # no constraint reads the last column
    Row("opening_zs_next",      OPENING,   ("zs_next", 1),    0, FRI_EVAL, FINAL_POLY),   # the batch opened at g * zeta
    Row("opening_pp",           OPENING,   ("pps", 9),        0, FRI_EVAL, FINAL_POLY),
    Row("opening_quotient",     OPENING,   ("quotient", -1),  0, FRI_EVAL, FINAL_POLY),   # absorbed by the compensation
    Row("fri_layer0_all",       FRI_LAYER, 0, 0,              FRI_EVAL,   None),
    Row("fri_layer1_all",       FRI_LAYER, 1, 0,              FRI_EVAL,   None),
    Row("fri_layer0_half",      FRI_LAYER, 0, 1,              FRI_EVAL,   None),
    Row("fri_layer1_half",      FRI_LAYER, 1, 1,              FRI_EVAL,   None),           # holds for query 0's index: see above
    Row("fri_fold0",            FRI_FOLD,  0, 0,              FRI_EVAL,   None),
    Row("fri_fold1",            FRI_FOLD,  1, 0,              FINAL_POLY, None),           # the last layer
    Row("final_poly_first",     FINAL,     0, 0,              FINAL_POLY, FINAL_POLY),
    Row("final_poly_last_imag", FINAL,     -1, 1,             FINAL_POLY, FINAL_POLY),     # second component only
)
SEEDS = {"flat": 5, "layers": 1}             # fri_layer1_half needs query 0 even at layer 1: seeds 1, 3, 5 and 7 give that

Forged = namedtuple("Forged", "name kind fault proof code")


def shape_of(c):
    n = Layout(c).n_layers
    assert n in (0, 2), "the table is written for the `and` gadget and its recursive verifier"
    return "layers" if n else "flat"


def section_sizes(c):
    i = c.info
    R, NC = int(i.num_routed_wires), int(i.num_challenges)
    return {"constants": int(i.num_constants_sigmas) - R, "sigmas": R, "wires": int(i.num_wires), "zs": NC, "zs_next": NC,
            "pps": NC * int(i.num_partial_products), "quotient": NC * int(i.quotient_degree_factor)}


def opening_index(c, section, k):
    sizes = section_sizes(c)
    k = k % sizes[section]
    assert section != "quotient" or k % int(c.info.quotient_degree_factor), "that element is the one the forgery solves for"
    return sum(sizes[s] for s in SECTIONS[:SECTIONS.index(section)]) + k


def fault_of(c, row):
    if row.kind == OPENING:
        return (OPENING, opening_index(c, *row.a), 0)
    if row.kind == FINAL:
        return (FINAL, row.a % Layout(c).final_poly_len, row.b)
    return (row.kind, row.a, row.b)


_forged = {}                                 # one forgery per (circuit, inputs, seed, row) and test session; read-only


def forge(oc, c, inputs, seed=None, kinds=None):
    """Every row of the table that applies to `c` (optionally of `kinds` only), forged by the oracle `oc` of `c`: a list
    of Forged with the table's code.  Rows that do not apply must be refused."""
    shape = shape_of(c)
    seed = SEEDS[shape] if seed is None else seed
    inputs = np.asarray(inputs, dtype=np.uint64)
    out = []
    for row in TABLE:
        if kinds is not None and row.kind not in kinds:
            continue
        key = (hash(c.to_blob()), inputs.tobytes(), seed, row.name)
        if key in _forged:
            out += _forged[key]
            continue
        fault, code = fault_of(c, row), getattr(row, shape)
        proof, st, msg = oc.prove_forged(inputs, seed, fault)
        if code is None:
            assert st == REFUSED and msg and not proof.any(), (row.name, st, msg)
            _forged[key] = []
            continue
        assert st == 0, (row.name, st, msg)
        proof.setflags(write=False)
        _forged[key] = [Forged(row.name, row.kind, fault, proof, code)]
        out += _forged[key]
    return out


def oracle_codes(oc, forged, dg, cap):
    return [expected(oc, f.proof, dg, cap) for f in forged]


def mixed(forged, honest, seed):
    """The forged proofs and as many honest ones in shuffled order: (batch, the table's codes, the rows' names)."""
    rows = [(f.proof, f.code, f.name) for f in forged] + [(honest, 0, "honest")] * len(forged)
    order = np.random.default_rng(seed).permutation(len(rows))
    return np.stack([rows[i][0] for i in order]), [rows[i][1] for i in order], [rows[i][2] for i in order]
