// The trace checker's per-row work, host and device (include/p25.h "CHECKING A TRACE"): the AIR's register program on the
// trace domain instead of the LDE coset.  The kernels of kernels_p3_check.hip only map lanes to (row, proof) and merge what
// the rows return; the host checker (p3_check.cpp) loops over the same functions, and everything here also compiles for the
// host alone (tests/native/p3_check_lanes.cpp).
//   check_row_lane     the constraints of one row: which of them are selected and non-zero
//   zero_den_lane      the first auxiliary column of one row whose denominator vanishes
//   last_terms_lane    t_j(n - 1) = num_j / den_j on the last row: what the running sums lack of the columns' totals
#pragma once
#include "p3_air_run.h"

namespace p25 {

// the report, in words (include/p25.h)
enum : uint32_t { P3CK_VERDICT = 0, P3CK_N_VIOLATIONS = 1, P3CK_FIRST_ROW = 2, P3CK_FIRST_CONSTRAINT = 3, P3CK_ZERO_ROW = 4,
                  P3CK_ZERO_COLUMN = 5, P3CK_TOTALS = 8 };
enum : uint32_t { P3CK_OK = 0, P3CK_VIOLATED = 1, P3CK_ZERO_DENOMINATOR = 2 };   // P25_P3_CHECK_*
constexpr uint32_t P3CK_NONE = 0xFFFFFFFFu;
GL_HD size_t p3ck_words(uint32_t AW, uint32_t n_constraints) { return P3CK_TOTALS + 2 * (size_t)AW + n_constraints; }

// What a handle decides of a check: the two programs and the tables they read by row.
struct P3CheckArgs {
  const P3Instr *prog, *aux_prog;
  const u64* consts;
  const u64* per_val;   // the periodic columns' values: the column with `off` words of columns before it at per_val + off
  const u64* pvals;     // the preprocessed columns on the trace domain [PW][n]
  uint32_t n_instr, n_aux_instr, n_constraints;
  uint32_t k, W, PW, AW, n_public;
};
// One proof: its trace in column form [W][n], its auxiliary columns [2 AW][n] (column j's components at 2 j and 2 j + 1; the
// running sums, so row 0 holds zeros), its public values and its challenges, two words each.  Whatever the AIR lacks is unread.
struct P3CheckProof {
  const u64 *tvals, *avals, *pub, *chal;
};

// A group of proofs on the device (kernels_p3_check.hip): proof g's buffers stand g strides behind these.  While the rows
// run, a report holds what they merge: the complement of the smallest violation key in word P3CK_FIRST_ROW and of the
// smallest zero-denominator key in word P3CK_ZERO_ROW (atomicMax over a zeroed word: 0 = none), the counts and the totals
// in their places; k_p3_check_finish turns that into the report.
struct P3CheckBatch {
  const u64 *tvals, *avals, *pub, *chal;   // strides W n, 2 AW n, n_public, chal_stride
  size_t chal_stride;
  const P3State* state;   // the term kernel's flag (status != 0: a zero denominator); read only with auxiliary columns
  u64* report;
  size_t report_stride;
};
// zeroes the reports' words on `st`, checks every row of G proofs, finishes the reports
void p3_launch_check(const P3CheckArgs& a, const P3CheckBatch& bt, uint32_t G, hipStream_t st);

namespace p3cklane {
using gl::E2;

GL_HD bool nonzero(u64 x) { return x != 0; }
GL_HD bool nonzero(E2 x) { return (x.a | x.b) != 0; }
// `when` on row i of n (AirProgram::When): always, the first row, the last row, every row but the last
GL_HD bool selected(uint32_t when, size_t i, size_t n) {
  return when == 0 || (when == 1 ? i == 0 : when == 2 ? i == n - 1 : i < n - 1);
}

template <class F>
struct Loader {
  const P3CheckArgs& a;
  const P3CheckProof& p;
  size_t n, i, i1;
  GL_HD typename F::T operator()(int which, uint32_t c) const {
    const size_t r = (which & 1) ? i1 : i;
    if constexpr (F::EXT) {
      if (which & 4) return E2{p.avals[(size_t)(2 * c) * n + r], p.avals[(size_t)(2 * c + 1) * n + r]};
    }
    return F::cst(((which & 2) ? a.pvals : p.tvals)[(size_t)c * n + r]);
  }
};
template <class F>
struct Periodic {
  const u64* per_val;
  size_t i;
  GL_HD typename F::T operator()(uint32_t x) const {
    return F::cst(per_val[p3_per_offset(x) + (i & (((size_t)1 << p3_per_log_period(x)) - 1))]);
  }
};

// Row i < n of proof p: runs the AIR's program and hands every constraint c, in the AIR's order, to visit(c, violated) --
// on every row alike, so the lanes of a wave call it together -- and returns the first violated c, or P3CK_NONE.  A row
// `live` = false (a lane past the trace's end, which reads row 0) violates nothing.
template <class F, class Visit>
GL_HD uint32_t check_row_lane(const P3CheckArgs& a, const P3CheckProof& p, size_t i, bool live, Visit visit) {
  const size_t n = (size_t)1 << a.k;
  uint32_t c = 0, first = P3CK_NONE;
  run_program<F>(a.prog, a.n_instr, a.consts, p.pub, p.chal, Loader<F>{a, p, n, i, (i + 1) & (n - 1)}, Periodic<F>{a.per_val, i},
                 [&](uint32_t when, const typename F::T& x) {
                   const bool bad = live && selected(when, i, n) && nonzero(x);
                   if (bad && first == P3CK_NONE) first = c;
                   visit(c, bad);
                   c++;
                 });
  return first;
}

// The terms' program on row i: num[j], den[j] for every auxiliary column.
GL_HD void aux_terms(const P3CheckArgs& a, const P3CheckProof& p, size_t i, E2* num, E2* den) {
  const size_t n = (size_t)1 << a.k;
  run_program<ExtF>(a.aux_prog, a.n_aux_instr, a.consts, p.pub, p.chal, Loader<ExtF>{a, p, n, i, (i + 1) & (n - 1)},
                    Periodic<ExtF>{a.per_val, i}, [&](uint32_t out, const E2& x) {
                      if (out & 1) den[out >> 1] = x;
                      else num[out >> 1] = x;
                    });
}
// the first auxiliary column whose denominator is zero on row i, or P3CK_NONE
GL_HD uint32_t zero_den_lane(const P3CheckArgs& a, const P3CheckProof& p, size_t i) {
  const size_t n = (size_t)1 << a.k;
  uint32_t first = P3CK_NONE;   // the program emits num_0, den_0, num_1, ... in column order: no array of them is kept
  run_program<ExtF>(a.aux_prog, a.n_aux_instr, a.consts, p.pub, p.chal, Loader<ExtF>{a, p, n, i, (i + 1) & (n - 1)},
                    Periodic<ExtF>{a.per_val, i}, [&](uint32_t out, const E2& x) {
                      if ((out & 1) && !nonzero(x) && first == P3CK_NONE) first = out >> 1;
                    });
  return first;
}
// total_j = S_j(n - 1) + num_j(n - 1) / den_j(n - 1), two words each to `totals`; the denominators are non-zero
GL_HD void last_terms_lane(const P3CheckArgs& a, const P3CheckProof& p, u64* totals) {
  const size_t n = (size_t)1 << a.k;
  E2 num[AirProgram::MAX_AUX], den[AirProgram::MAX_AUX];
  aux_terms(a, p, n - 1, num, den);
  for (uint32_t j = 0; j < a.AW; j++) {
    const E2 s = E2{p.avals[(size_t)(2 * j) * n + n - 1], p.avals[(size_t)(2 * j + 1) * n + n - 1]};
    const E2 t = gl::add(s, gl::mul(num[j], gl::inv(den[j])));
    totals[2 * j] = t.a;
    totals[2 * j + 1] = t.b;
  }
}

// What the rows of a proof left in its report, turned into the report: `first` and `zero` are the smallest keys
// row * n_constraints + c and row * AW + column found (found_first / found_zero: whether any was), the counts stand in
// place.  A zero denominator leaves everything else at its "none" value.
GL_HD void finish_lane(const P3CheckArgs& a, u64* rep, bool found_first, u64 first, bool found_zero, u64 zero) {
  const uint32_t o_counts = P3CK_TOTALS + 2 * a.AW;
  rep[6] = rep[7] = 0;
  if (found_zero) {
    rep[P3CK_VERDICT] = P3CK_ZERO_DENOMINATOR;
    rep[P3CK_N_VIOLATIONS] = 0;
    rep[P3CK_FIRST_ROW] = rep[P3CK_FIRST_CONSTRAINT] = ~(u64)0;
    rep[P3CK_ZERO_ROW] = zero / a.AW;
    rep[P3CK_ZERO_COLUMN] = zero % a.AW;
    for (uint32_t j = 0; j < 2 * a.AW + a.n_constraints; j++) rep[P3CK_TOTALS + j] = 0;
    return;
  }
  u64 sum = 0;
  for (uint32_t c = 0; c < a.n_constraints; c++) sum += rep[o_counts + c];
  rep[P3CK_VERDICT] = found_first ? P3CK_VIOLATED : P3CK_OK;
  rep[P3CK_N_VIOLATIONS] = sum;
  rep[P3CK_FIRST_ROW] = found_first ? first / a.n_constraints : ~(u64)0;
  rep[P3CK_FIRST_CONSTRAINT] = found_first ? first % a.n_constraints : ~(u64)0;
  rep[P3CK_ZERO_ROW] = rep[P3CK_ZERO_COLUMN] = ~(u64)0;
}

}  // namespace p3cklane
}  // namespace p25
