// Checking a trace against its AIR on the device (include/p25.h "CHECKING A TRACE"): the AIR's register program on the
// trace domain, one lane per (row, proof).  The per-row work is p3_check_lanes.h, which the host checker runs too; the
// kernels map lanes to rows and merge what the rows find:
//   counts    the program is the same for every lane, so every constraint is reached by the whole wave at once: the wave
//             ballots "violated" and ONE lane adds the popcount, and only when a lane voted
//   first     the lanes of a wave hold consecutive rows, so the wave's smallest key row * n_constraints + c is the one of
//             its lowest lane that found anything: that lane alone issues the wave's atomic
// The keys are merged as their complements by atomicMax over words the launcher has zeroed (0 = none).
#include "dev_res.h"
#include "p3_check_lanes.h"

namespace p25 {
namespace {

__device__ __forceinline__ unsigned long long* ull(u64* p) { return reinterpret_cast<unsigned long long*>(p); }

__device__ __forceinline__ P3CheckProof proof_of(const P3CheckArgs& a, const P3CheckBatch& bt, uint32_t g) {
  const size_t n = (size_t)1 << a.k;
  P3CheckProof p;
  p.tvals = bt.tvals + (size_t)g * a.W * n;
  p.avals = a.AW ? bt.avals + (size_t)g * 2 * a.AW * n : nullptr;
  p.pub = a.n_public ? bt.pub + (size_t)g * a.n_public : nullptr;
  p.chal = a.AW ? bt.chal + (size_t)g * bt.chal_stride : nullptr;
  return p;
}

// F = BaseF: an AIR without auxiliary columns.  F = ExtF: one with them, evaluated in F_p^2 throughout as the prover does.
// A proof whose term kernel met a zero denominator has no running sums: its rows only locate the first such denominator.
template <class F>
__global__ __launch_bounds__(256) void k_p3_check(P3CheckArgs a, P3CheckBatch bt) {
  const size_t n = (size_t)1 << a.k, row = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = row < n;
  const size_t i = live ? row : 0;   // a lane past the end runs row 0 and reports nothing: the wave stays whole
  const uint32_t g = blockIdx.y, lane = threadIdx.x & 63;
  const P3CheckProof p = proof_of(a, bt, g);
  u64* rep = bt.report + (size_t)g * bt.report_stride;
  if constexpr (F::EXT) {
    if (bt.state[g].status != 0) {   // uniform over the block
      const uint32_t col = live ? p3cklane::zero_den_lane(a, p, i) : P3CK_NONE;
      const unsigned long long m = __ballot(col != P3CK_NONE);
      if (m != 0 && lane == (uint32_t)(__ffsll((long long)m) - 1)) atomicMax(ull(rep + P3CK_ZERO_ROW), ~((u64)i * a.AW + col));
      return;
    }
  }
  u64* counts = rep + P3CK_TOTALS + 2 * a.AW;
  const uint32_t first = p3cklane::check_row_lane<F>(a, p, i, live, [&](uint32_t c, bool bad) {
    const unsigned long long m = __ballot(bad);
    if (m != 0 && lane == 0) atomicAdd(ull(counts + c), (unsigned long long)__popcll(m));
  });
  const unsigned long long m = __ballot(first != P3CK_NONE);
  if (m != 0 && lane == (uint32_t)(__ffsll((long long)m) - 1))
    atomicMax(ull(rep + P3CK_FIRST_ROW), ~((u64)i * a.n_constraints + first));
}

// One lane per proof: the keys decoded, the counts summed, the verdict -- and the totals, which are one lane's work per
// proof (the last row's terms on top of the last running sums) and so stay out of the wide kernel.
__global__ __launch_bounds__(64) void k_p3_check_finish(P3CheckArgs a, P3CheckBatch bt, uint32_t G) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  u64* rep = bt.report + (size_t)g * bt.report_stride;
  const u64 first = rep[P3CK_FIRST_ROW], zero = rep[P3CK_ZERO_ROW];
  if (a.AW && zero == 0) p3cklane::last_terms_lane(a, proof_of(a, bt, g), rep + P3CK_TOTALS);   // no running sums otherwise
  p3cklane::finish_lane(a, rep, first != 0, ~first, zero != 0, ~zero);
}
}  // namespace

void p3_launch_check(const P3CheckArgs& a, const P3CheckBatch& bt, uint32_t G, hipStream_t st) {
  const size_t n = (size_t)1 << a.k, words = p3ck_words(a.AW, a.n_constraints);
  P25_HIP(hipMemset2DAsync(bt.report, bt.report_stride * 8, 0, words * 8, G, st));
  const dim3 grid((unsigned)((n + 255) / 256), G);
  if (a.AW) hipLaunchKernelGGL(k_p3_check<ExtF>, grid, dim3(256), 0, st, a, bt);
  else hipLaunchKernelGGL(k_p3_check<BaseF>, grid, dim3(256), 0, st, a, bt);
  hipLaunchKernelGGL(k_p3_check_finish, dim3((G + 63) / 64), dim3(64), 0, st, a, bt, G);
}

}  // namespace p25
