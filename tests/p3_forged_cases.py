"""Forged plonky3 proofs from the model prover (tests/p3_prove_model.py): the shapes, the fault table and the forged sets.

A flipped word of a finished proof is caught by the first check that reads the word.  A cheating prover sends something
else: a proof finished HONESTLY from faulted data, in which every commitment, opening, FRI layer and path is consistent and
exactly one check fails.  The codes are written down from the documented order of checks (include/p25.h "Verifying inner
plonky3 proofs", DESIGN 7.2 and 7.7: a word >= p 30, the proof of work 31, the input openings of every query 32, then per
query its FRI Merkle openings 33 and its comparison with final_poly 34, the identity at zeta 35 LAST), never read from a
verifier:

  row(r, c)        trace cell bumped before anything is committed; the quotient is C / Z_H on the quotient coset,
                   interpolated as usual: everything is consistent, only the identity at zeta fails                  -> 35
  unbalanced       a lookup / permutation trace whose terms do not sum to zero; the running sums from their definition -> 35
  aux_start(j)     auxiliary column j starts at 1, the trace is honest                                                 -> 35
  chunk(c, comp)   1 added to coefficient 0 of quotient chunk c, component comp, before the quotient commitment        -> 35
  public(i)        the trace was built for another value of PUBLIC(i) than the one sent and observed                   -> 35
  opened(sec, i)   1 added to word i of an opened section after zeta; the reduced openings, every FRI layer and
                   final_poly = layer[0] follow honestly: the last layer is not constant, and the first query whose final
                   position is not 0 fails its comparison                                                              -> 34
  fold(r)          1 added to every entry of FRI layer r + 1 before it is committed: query 0's leaf of round r + 1 holds
                   a value that is not the fold of round r                                                             -> 33
  final(comp)      final_poly's component bumped                                                                       -> 34

35 is the last key: a forged proof that gets 35 from the model fails exactly one check.

For the faults that are a property of the TRACE (row, unbalanced, public) and for aux_start the table also names the pair
(row, constraint) the trace checker must report first -- written down from the AIRs of tests/air_cases*.py, each reason
beside it -- which ties "the check says where", "the prover refuses" and "the verifier rejects" to the same data.

The `opened` rows need a query whose final position index >> log_n is not 0 (else every comparison reads layer[0] itself)
and a zeta outside the base field.  pow_start moves the query indices; POW_START holds the value chosen per shape and per
forgery where the shape's own does not do, and build() asserts the precondition from the model's sampled indices."""
from collections import namedtuple

import numpy as np

import air_cases_aux
import air_cases_periodic
import air_cases_preprocessed
import air_cases_pv
import p3_aux_model as M
import p3_prove_model as PV
import p3_verify_cases

P = M.P
Spec = namedtuple("Spec", "make queries pow_bits rows unbalanced aux_start public")
Forged = namedtuple("Forged", "name kind fault proof code trace pv first indices")


def _plain(name):
    return lambda p25: p3_verify_cases.air_and_trace(p25, name, 3) + (None, 3, {"fib": 1, "cubic": 1, "quartic_map:6": 2}[name])


def _fib_pv(p25):
    trace, pv = air_cases_pv.fib_pv_trace(3, 3, 5)
    return air_cases_pv.fib_pv(p25), trace, pv, 3, 1


def _mimc(p25):
    return air_cases_periodic.make(p25, air_cases_periodic.SHAPES[air_cases_periodic.SHAPE_IDS.index("mimc2_2")])


def _machine(p25):
    air, trace, pv, _prep, log_n, log_blowup = air_cases_preprocessed.make(p25, air_cases_preprocessed.shape("machine2"))
    return air, trace, pv, log_n, log_blowup


def _aux(name):
    return lambda p25: air_cases_aux.make(p25, air_cases_aux.shape(name))


def _bump_last_column(trace):
    """A wrong multiplicity (the last column of range / tuple / pvper) on row 1."""
    bad = trace.copy()
    bad[1, -1] = (int(bad[1, -1]) + 1) % P
    return bad


# rows: ((r, c) bumped, (row, constraint) the checker reports first).  Constraint 0 carries the highest alpha power, the last
# one the lowest.  n = 8 rows, or 16 for range and pvper.
_FIB_ROWS = (((0, 0), (0, 0)),      # a on the first row: the sum (always, 0) and a = 1 (first row, 1), both on row 0
             ((7, 2), (7, 0)),      # c on the last row: the sum alone (no transition constraint is selected there)
             ((4, 1), (3, 4)))      # b on row 4: next b - c on row 3 (transition, the LAST constraint), then rows 4's
_MAP_ROWS = (((0, 0), (0, 0)),      # x on the first row: y = f(x) (always, 0) and x = x0 (first row, 1)
             ((7, 1), (7, 0)),      # y on the last row: y = f(x) alone
             ((3, 0), (2, 2)))      # x on row 3: next x (transition, the last constraint) on row 2
_CHAIN_ROWS = (((0, 0), (0, 0)),    # width 1, first row x = pv0 (0) | transition (1) | last row x = pv1 (2): x on row 0
               ((4, 0), (3, 1)),    # x on row 4: the transition into it
               ((7, 0), (6, 1)))    # x on the last row: the transition into it first, then x = pv1 on row 7
_CHAIN_PUBLIC = ((0, (0, 0)), (1, (7, 2)))       # pv0 is read on the first row alone, pv1 on the last (the lowest power)
# the usual pair per auxiliary column: first row AUX_LOCAL = 0, every row (AUX_NEXT - AUX_LOCAL) den - num = 0.  The sums
# follow their definition on rows 0..n-2 whatever the trace holds; the cyclic last row sees a total that is not zero.
SPECS = {
    "fib": Spec(_plain("fib"), 3, 4, _FIB_ROWS, None, (), ()),
    "cubic": Spec(_plain("cubic"), 2, 3, _MAP_ROWS, None, (), ()),
    "quartic_map": Spec(_plain("quartic_map:6"), 2, 3, _MAP_ROWS, None, (), ()),
    # fib with first row a = pv0 (1), b = pv1 (2) and last row c = pv2 (5)
    "fib_pv": Spec(_fib_pv, 3, 4, (((0, 0), (0, 0)), ((7, 2), (7, 0)), ((4, 1), (3, 4))), None, (),
                   ((0, (0, 1)), (2, (7, 5)))),
    "mimc": Spec(_mimc, 3, 4, _CHAIN_ROWS, None, (), _CHAIN_PUBLIC),
    "machine": Spec(_machine, 3, 4, _CHAIN_ROWS, None, (), _CHAIN_PUBLIC),
    "perm": Spec(_aux("perm"), 3, 4, (((2, 0), (7, 1)),), (air_cases_aux.not_a_permutation, (7, 1)), ((0, (0, 0)),), ()),
    "range": Spec(_aux("range"), 3, 4, (((3, 0), (15, 1)),), (_bump_last_column, (15, 1)), ((0, (0, 0)),), ()),
    # two columns: first row (0), every row (1) of column 0, then (2), (3) of column 1; x enters both
    "tuple": Spec(_aux("tuple"), 3, 4, (((2, 0), (7, 1)),), (_bump_last_column, (7, 1)), ((0, (0, 0)), (1, (0, 2))), ()),
    # first row f = pv1 (0), then the pair (1), (2).  pv0 only shifts the challenge: a lookup is balanced under any shift
    "pvper": Spec(_aux("pvper"), 3, 4, (((0, 0), (0, 0)), ((5, 1), (15, 2))), (_bump_last_column, (15, 2)), ((0, (0, 1)),),
                  ((1, (0, 0)),)),
    "perm_b2": Spec(_aux("perm_b2"), 3, 4, (((2, 0), (7, 1)),), (air_cases_aux.not_a_permutation, (7, 1)), ((0, (0, 0)),), ()),
}
SHAPE_IDS = list(SPECS)
RECURSION_IDS = ("fib", "range")
# pow_start per shape, and per forgery where the shape's own leaves every query at final position 0 (see the docstring)
POW_START = {name: 0 for name in SPECS}
POW_START_OF = {
    ("fib", "opened(chunks, -1)"): 11, ("cubic", "opened(trace_next, -1)"): 2, ("quartic_map", "opened(chunks, 0)"): 5,
    ("fib_pv", "opened(trace_next, -1)"): 17, ("mimc", "opened(trace_local, -1)"): 10, ("mimc", "opened(trace_next, -1)"): 1,
    ("perm", "opened(trace_next, -1)"): 11, ("range", "opened(prep_next, 0)"): 12, ("range", "opened(aux_local, -1)"): 26,
    ("tuple", "opened(trace_local, -1)"): 4, ("tuple", "opened(aux_local, 0)"): 11, ("pvper", "opened(trace_next, -1)"): 14,
}
SECTIONS = ("trace_local", "trace_next", "chunks", "prep_local", "prep_next", "aux_local", "aux_next")


def fault_name(fault):
    return "%s(%s)" % (fault[0], ", ".join(str(v) for v in fault[1:]))


class Built:
    """One shape: air, trace, pv, log_n, log_blowup, queries, pow_bits, the honest proof (p3_prove_model.Proof), prep_commit
    and forged = [Forged]."""

    def verify(self, oracle, words, air=None):
        return M.verify(oracle, air or self.air, self.cfg, words, self.prep_commit)


_built = {}


def build(p25, oracle, name):
    """The shape's honest proof and its forged set, made once per session and read-only."""
    if name in _built:
        return _built[name]
    spec = SPECS[name]
    b = Built()
    b.name, b.queries, b.pow_bits = name, spec.queries, spec.pow_bits
    b.air, b.trace, b.pv, b.log_n, b.log_blowup = spec.make(p25)
    b.pow_start = POW_START[name]

    def prove(trace, pv, fault=None, pow_start=b.pow_start):
        return PV.prove(oracle, b.air, trace, b.log_blowup, b.queries, b.pow_bits, pow_start, pv, fault)
    b.honest = prove(b.trace, b.pv)
    b.cfg, b.shape, b.prep_commit = b.honest.cfg, b.honest.shape, b.honest.prep_commit
    b.words = b.honest.words
    b.words.setflags(write=False)
    s, k = b.shape, b.log_n
    out = []

    def add(kind, fault, code, trace=None, pv=None, first=None, label=None):
        label = label or fault_name(fault)
        trace = b.trace if trace is None else trace
        pv = b.pv if pv is None else pv
        p = prove(trace, pv, fault if kind not in ("unbalanced", "public") else None, POW_START_OF.get((name, label), b.pow_start))
        if kind == "opened":                                 # the precondition, from the model's own indices
            assert p.zeta[1] != 0 and any(i >> k for i in p.indices), (name, label, p.indices)
        p.words.setflags(write=False)
        out.append(Forged(label, kind, fault, p.words, code, trace, pv, first, tuple(p.indices)))

    for (r, c), first in spec.rows:
        bad = b.trace.copy()
        bad[r, c] = (int(bad[r, c]) + 1) % P
        add("row", ("row", r, c), M.CONSTRAINTS, first=first)
        out[-1] = out[-1]._replace(trace=bad)                # the trace as the prover saw it
    if spec.unbalanced:
        make_bad, first = spec.unbalanced
        add("unbalanced", ("unbalanced",), M.CONSTRAINTS, trace=make_bad(b.trace), first=first)
    for j, first in spec.aux_start:
        add("aux_start", ("aux_start", j), M.CONSTRAINTS, first=first)
    for i, first in spec.public:
        sent = b.pv.copy()
        sent[i] = (int(sent[i]) + 1) % P
        add("public", ("public", i), M.CONSTRAINTS, pv=sent, first=first)
    for c in sorted({0, s.Q - 1}):
        for comp in (0, 1):
            add("chunk", ("chunk", c, comp), M.CONSTRAINTS)
    for r in sorted({0, k - 2}):
        add("fold", ("fold", r), M.FRI_MERKLE)
    widths = {"trace_local": s.W, "trace_next": s.W, "chunks": 2 * s.Q, "prep_local": s.PW, "prep_next": s.PW,
              "aux_local": 2 * s.AW, "aux_next": 2 * s.AW}
    for sec in SECTIONS:
        for i in ((0, -1) if widths[sec] else ()):
            add("opened", ("opened", sec, i), M.FINAL_POLY)
    for comp in (0, 1):
        add("final", ("final", comp), M.FINAL_POLY)
    b.forged = out
    _built[name] = b
    return b


def mixed(forged, honest, seed):
    """The forged proofs and as many honest ones in shuffled order: (batch, the table's codes, the rows' names)."""
    rows = [(f.proof, f.code, f.name) for f in forged] + [(honest, 0, "honest")] * len(forged)
    order = np.random.default_rng(seed).permutation(len(rows))
    return np.stack([rows[i][0] for i in order]), [rows[i][1] for i in order], [rows[i][2] for i in order]


def _with(words, pos, value=None):
    """A copy with bit 0 of word `pos` flipped, or the word set to `value`."""
    w = np.array(words, dtype=np.uint64)
    w[pos] = np.uint64(value) if value is not None else w[pos] ^ np.uint64(1)
    return w


def precedence(b):
    """name -> (proof, code): two failures in one proof, the verdict is the earlier key's.  Written down from the key order;
    for a shape with 3 queries.  `b.forged` supplies the 35-forgery (its first row fault), fold(0) and an opened forgery."""
    assert b.queries == 3
    s = b.shape
    f35 = next(f for f in b.forged if f.code == M.CONSTRAINTS).proof
    fold0 = next(f for f in b.forged if f.name == "fold(0)").proof
    out = {
        "35 + input path of query 2": (_with(f35, s.opening(2, 0) + s.W + 1), M.INPUT_MERKLE),
        "35 + FRI sibling of query 1": (_with(f35, s.step(1, 0)), M.FRI_MERKLE),
        "35 + final_poly": (_with(f35, s.o_final_poly, (int(f35[s.o_final_poly]) + 1) % P), M.FINAL_POLY),
        "35 + word = p": (_with(f35, s.o_trace_next + 1, P), M.MALFORMED),
        "fold(0) + round-0 path of query 0": (_with(fold0, s.step(0, 0) + 2), M.FRI_MERKLE),
    }
    # an opened forgery whose first failing query is not the last: a FRI path flipped in a LATER query changes nothing
    for f in b.forged:
        if f.kind != "opened":
            continue
        q = next(q for q, i in enumerate(f.indices) if i >> b.log_n)
        if q < b.queries - 1:
            out["%s (fails at query %d) + FRI path of query %d" % (f.name, q, q + 1)] = (_with(f.proof, s.step(q + 1, 0) + 3), M.FINAL_POLY)
            break
    else:
        raise AssertionError("no opened forgery of %s fails before the last query" % b.name)
    return out
