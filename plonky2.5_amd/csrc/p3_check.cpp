// The host checker of a trace against its AIR (include/p25.h "CHECKING A TRACE"): plain loops over the per-row functions
// of p3_check_lanes.h, which the device's kernels (kernels_p3_check.hip) call for one row each.  Works without a GPU.
#include <stdexcept>
#include "p3_check_lanes.h"
#include "p3_prover.h"

namespace p25 {

std::vector<u64> p3_check_air(const AirProgram& air, const std::vector<std::vector<u64>>& col, const std::vector<u64>& pub,
                              int log_n, int log_blowup, int threads) {
  p3_check_params(air, log_n, log_blowup, 1, 0);
  const size_t n = (size_t)1 << log_n, W = (size_t)air.width, PW = air.prep.width, AW = air.aux.width();
  if (col.size() != W) throw std::invalid_argument("p3_check: trace width does not match the AIR");
  if ((int)pub.size() != air.n_public) throw std::invalid_argument("p3_check: the AIR takes n_public public values");
  for (u64 v : pub)
    if (v >= gl::P) throw std::invalid_argument("p3_check: non-canonical public value");
  std::vector<u64> tvals(W * n), pvals(PW * n), avals(2 * AW * n, 0);
  for (size_t c = 0; c < W; c++) {
    if (col[c].size() != n) throw std::invalid_argument("p3_check: trace height does not match log_n");
    for (size_t r = 0; r < n; r++) {
      if (col[c][r] >= gl::P) throw std::invalid_argument("p3_check: non-canonical trace value");
      tvals[c * n + r] = col[c][r];
    }
  }
  for (size_t r = 0; r < n; r++)
    for (size_t c = 0; c < PW; c++) pvals[c * n + r] = air.prep.values[r * PW + c];

  // the handle's host half: the two programs, their constants and the periodic values
  const P3ProverDev dev(air, log_n, log_blowup, 1, 0);
  P3CheckArgs a = dev.check_args();
  a.pvals = pvals.data();
  std::vector<u64> chal;
  for (const gl::E2& c : p3_trace_challenges(air, col, pub, log_n, log_blowup, threads)) {
    chal.push_back(c.a);
    chal.push_back(c.b);
  }
  const P3CheckProof p{tvals.data(), avals.data(), pub.data(), chal.data()};
  std::vector<u64> rep(dev.check_words(), 0);

  // one pass over the terms' program: the first zero denominator in (row, column) order ends the check; otherwise the
  // running sums, one inversion a row (Montgomery's trick over the row's AW denominators, as the prover's term kernel)
  std::vector<gl::E2> run(AW, gl::e2(0));
  if (AW) {
    gl::E2 num[AirProgram::MAX_AUX], den[AirProgram::MAX_AUX], pre[AirProgram::MAX_AUX];
    for (size_t i = 0; i < n; i++) {
      for (size_t j = 0; j < AW; j++) {
        avals[2 * j * n + i] = run[j].a;
        avals[(2 * j + 1) * n + i] = run[j].b;
      }
      p3cklane::aux_terms(a, p, i, num, den);
      gl::E2 acc = gl::e2(1);
      for (size_t j = 0; j < AW; j++) {
        if (!p3cklane::nonzero(den[j])) {
          p3cklane::finish_lane(a, rep.data(), false, 0, true, (u64)i * AW + j);
          return rep;
        }
        pre[j] = acc;
        acc = gl::mul(acc, den[j]);
      }
      gl::E2 inv = gl::inv(acc);
      for (size_t j = AW; j-- > 0;) {
        run[j] = gl::add(run[j], gl::mul(num[j], gl::mul(inv, pre[j])));
        inv = gl::mul(inv, den[j]);
      }
    }
  }
  u64* counts = rep.data() + P3CK_TOTALS + 2 * AW;
  auto count = [&](uint32_t c, bool bad) { counts[c] += bad ? 1 : 0; };
  bool found = false;
  u64 first = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t c = AW ? p3cklane::check_row_lane<ExtF>(a, p, i, true, count) : p3cklane::check_row_lane<BaseF>(a, p, i, true, count);
    if (c != P3CK_NONE && !found) {
      found = true;
      first = (u64)i * a.n_constraints + c;
    }
  }
  for (size_t j = 0; j < AW; j++) {   // the sums past the last row: the columns' totals (the device: last_terms_lane)
    rep[P3CK_TOTALS + 2 * j] = run[j].a;
    rep[P3CK_TOTALS + 2 * j + 1] = run[j].b;
  }
  p3cklane::finish_lane(a, rep.data(), found, first, false, 0);
  return rep;
}

}  // namespace p25
