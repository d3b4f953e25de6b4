// The trace checker's lane functions (plonky2.5_amd/csrc/p3_check_lanes.h) in plain loops, as a stand-alone host program:
// what k_p3_check does with one lane per row, here row after row -- in DESCENDING order, so that "first" is a minimum and
// not an arrival order.  The challenges come with the data: the program runs no transcript.
//   p3_check_lanes <data>   data (u64 words) = width | n_nodes | n_constraints | log_n | log_blowup | n_public |
//                           n_challenges | aux width | n_periodic | prep width | nodes[n_nodes][op, a, b, value] |
//                           constraints[n_constraints][node, when] | columns[aux width][num, den] |
//                           periodic[n_periodic]{log_period, values[2^log_period]} | prep[2^log_n][prep width] |
//                           public[n_public] | challenges[n_challenges][2] | trace[2^log_n][width]
// prints the report, one word per line.  Linked against libp25.so for the AIR's compilation only.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "p3_check_lanes.h"

using namespace p25;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<u64> w;
  u64 buf[1 << 13];
  size_t got;
  while ((got = fread(buf, 8, 1 << 13, f)) > 0) w.insert(w.end(), buf, buf + got);
  fclose(f);
  if (w.size() < 10) return 2;
  AirProgram air;
  air.width = (int)w[0];
  const size_t n_nodes = w[1], n_cons = w[2], k = w[3], n_public = w[5], nc = w[6], aw = w[7], n_per = w[8], pw = w[9];
  const size_t n = (size_t)1 << k;
  air.n_public = (int)n_public;
  air.aux.n_challenges = (uint32_t)nc;
  size_t at = 10;
  auto need = [&](size_t words) {
    if (at + words > w.size()) {
      fprintf(stderr, "data file too short\n");
      exit(2);
    }
  };
  need(4 * n_nodes + 2 * n_cons + 2 * aw);
  for (size_t i = 0; i < n_nodes; i++, at += 4)
    air.nodes.push_back(AirProgram::Node{(uint32_t)w[at], (uint32_t)w[at + 1], (uint32_t)w[at + 2], w[at + 3]});
  for (size_t i = 0; i < n_cons; i++, at += 2) air.constraints.push_back(AirProgram::Constraint{(uint32_t)w[at], (uint32_t)w[at + 1]});
  for (size_t i = 0; i < aw; i++, at += 2) air.aux.columns.push_back(AirProgram::AuxColumn{(uint32_t)w[at], (uint32_t)w[at + 1]});
  for (size_t c = 0; c < n_per; c++) {
    need(1);
    AirProgram::Periodic pc;
    pc.log_period = (uint32_t)w[at++];
    need((size_t)1 << pc.log_period);
    pc.values.assign(w.begin() + at, w.begin() + at + ((size_t)1 << pc.log_period));
    at += pc.values.size();
    air.periodic.push_back(pc);
  }
  need(pw * n + n_public + 2 * nc + (size_t)air.width * n);
  if (pw) {
    air.prep.width = (uint32_t)pw;
    air.prep.log_n = (uint32_t)k;
    air.prep.values.assign(w.begin() + at, w.begin() + at + pw * n);
    at += pw * n;
  }
  const std::vector<u64> pub(w.begin() + at, w.begin() + at + n_public);
  at += n_public;
  const std::vector<u64> chal(w.begin() + at, w.begin() + at + 2 * nc);
  at += 2 * nc;
  if (w.size() != at + (size_t)air.width * n) {
    fprintf(stderr, "data file has the wrong size\n");
    return 2;
  }
  const size_t W = (size_t)air.width;
  // exactly-sized heap arrays in column form: a read past a column's end is the sanitizer's to find
  std::vector<u64> tvals(W * n), pvals(pw * n), avals(2 * aw * n);
  for (size_t r = 0; r < n; r++) {
    for (size_t c = 0; c < W; c++) tvals[c * n + r] = w[at + r * W + c];
    for (size_t c = 0; c < pw; c++) pvals[c * n + r] = air.prep.values[r * pw + c];
  }

  const P3ProverDev dev(air, (int)k, (int)w[4], 1, 0);
  P3CheckArgs a = dev.check_args();
  a.pvals = pvals.data();
  const P3CheckProof p{tvals.data(), avals.data(), pub.data(), chal.data()};
  std::vector<u64> rep(dev.check_words(), 0);
  if (rep.size() != p3ck_words((uint32_t)aw, (uint32_t)n_cons)) return 3;

  bool found_zero = false, found = false;
  u64 zero = 0, first = 0;
  if (aw) {
    for (size_t i = n; i-- > 0;) {
      const uint32_t j = p3cklane::zero_den_lane(a, p, i);
      if (j != P3CK_NONE && (!found_zero || (u64)i * aw + j < zero)) {
        found_zero = true;
        zero = (u64)i * aw + j;
      }
    }
    if (!found_zero) {   // the running sums, as the scan leaves them
      std::vector<gl::E2> run(aw, gl::e2(0));
      gl::E2 num[AirProgram::MAX_AUX], den[AirProgram::MAX_AUX];
      for (size_t i = 0; i < n; i++) {
        for (size_t j = 0; j < aw; j++) {
          avals[2 * j * n + i] = run[j].a;
          avals[(2 * j + 1) * n + i] = run[j].b;
        }
        p3cklane::aux_terms(a, p, i, num, den);
        for (size_t j = 0; j < aw; j++) run[j] = gl::add(run[j], gl::mul(num[j], gl::inv(den[j])));
      }
    }
  }
  if (!found_zero) {
    u64* counts = rep.data() + P3CK_TOTALS + 2 * aw;
    auto count = [&](uint32_t c, bool bad) {
      if (c >= n_cons) abort();
      counts[c] += bad ? 1 : 0;
    };
    for (size_t i = n; i-- > 0;) {
      const uint32_t c = aw ? p3cklane::check_row_lane<ExtF>(a, p, i, true, count) : p3cklane::check_row_lane<BaseF>(a, p, i, true, count);
      if (c != P3CK_NONE && (!found || (u64)i * n_cons + c < first)) {
        found = true;
        first = (u64)i * n_cons + c;
      }
    }
    // a lane past the trace's end runs row 0 and must report nothing
    auto silent = [](uint32_t, bool bad) {
      if (bad) abort();
    };
    if ((aw ? p3cklane::check_row_lane<ExtF>(a, p, 0, false, silent) : p3cklane::check_row_lane<BaseF>(a, p, 0, false, silent)) != P3CK_NONE)
      abort();
    if (aw) p3cklane::last_terms_lane(a, p, rep.data() + P3CK_TOTALS);
  }
  p3cklane::finish_lane(a, rep.data(), found, first, found_zero, zero);
  for (u64 v : rep) printf("%llu\n", (unsigned long long)v);
  return 0;
}
