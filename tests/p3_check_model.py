"""The report of a trace check (include/p25.h "CHECKING A TRACE") from its definition, in plain Python over integers.

Written from the header's statement, not from the library's code, on top of tests/p3_aux_model.py: eval_nodes evaluates the
DAG on one row, running_sums states the auxiliary columns, challenges_of the transcript.  A rejected trace has no proof, so
the challenges come from `root | public values`, the root being the commit the trace gets: the models' own MMCS
(p3_preprocessed_model.model_commit, quadratic in the height) up to 16 rows, and above that the library's host function
p25_p3_preprocessed_commit applied to the trace as a matrix, which the header names as that commit and
tests/test_p3_preprocessed_cpu.py holds against the same model.

report(...) -> the words: verdict | violations | first row, constraint | zero row, column | 0, 0 | totals | counts."""
import numpy as np

import p3_preprocessed_model as PM
from p3_aux_model import challenges_of, eval_nodes, running_sums
from p3_verify_model import e, e_add, e_inv, e_mul

OK, VIOLATED, ZERO_DENOMINATOR = 0, 1, 2
NONE = (1 << 64) - 1
MODEL_COMMIT_MAX_ROWS = 16


def selected(when, i, n):
    return when == 0 or (when == 1 and i == 0) or (when == 2 and i == n - 1) or (when == 3 and i < n - 1)


def trace_root(oracle, p25, trace, log_blowup):
    if trace.shape[0] <= MODEL_COMMIT_MAX_ROWS:
        return PM.model_commit(oracle, trace, log_blowup)
    return [int(v) for v in p25.p3_preprocessed_commit(trace, log_blowup, threads=1)]


def challenges(oracle, p25, air, trace, pv, log_blowup):
    if not air.n_challenges:
        return []
    key = None
    if air.preprocessed is not None:
        prep = np.asarray(air.preprocessed, dtype=np.uint64)
        key = trace_root(oracle, p25, prep, log_blowup)
    return challenges_of(oracle, air, trace_root(oracle, p25, trace, log_blowup) + pv, None, key)


def report(oracle, p25, air, trace, public_values=None, log_blowup=1):
    trace = np.asarray(trace, dtype=np.uint64)
    n, aw, nc = trace.shape[0], len(air.aux_columns), len(air.constraints)
    pv = [int(v) for v in public_values] if public_values is not None else []
    chal = challenges(oracle, p25, air, trace, pv, log_blowup) if aw else []
    rows = [[e(int(x)) for x in r] for r in trace]
    prep = None if air.preprocessed is None else [[e(int(x)) for x in r] for r in air.preprocessed]

    def row_values(i, aux_local, aux_next):
        i1 = (i + 1) % n
        per = [e(int(c[i % len(c)])) for c in air.periodic_columns]
        return eval_nodes(air, rows[i], rows[i1], pv, per, prep[i] if prep else None, prep[i1] if prep else None, chal,
                          aux_local, aux_next)

    for i in range(n) if aw else ():
        v = row_values(i, None, None)
        for j, (_nu, de) in enumerate(air.aux_columns):
            if v[de] == e(0):
                return [ZERO_DENOMINATOR, 0, NONE, NONE, i, j, 0, 0] + [0] * (2 * aw + nc)
    sums = running_sums(air, trace, pv, chal) if aw else None
    counts, first = [0] * nc, None
    for i in range(n):
        v = row_values(i, sums[i] if aw else None, sums[(i + 1) % n] if aw else None)
        for c, (node, when) in enumerate(air.constraints):
            if selected(when, i, n) and v[node] != e(0):
                counts[c] += 1
                if first is None:
                    first = (i, c)
    totals = []
    if aw:
        v = row_values(n - 1, None, None)
        for j, (nu, de) in enumerate(air.aux_columns):
            totals += list(e_add(sums[n - 1][j], e_mul(v[nu], e_inv(v[de]))))
    head = [VIOLATED if first else OK, sum(counts)] + (list(first) if first else [NONE, NONE]) + [NONE, NONE, 0, 0]
    return head + [int(t) for t in totals] + counts
