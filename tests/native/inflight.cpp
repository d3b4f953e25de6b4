// Stand-alone check of inflight.h (no GPU, no HIP): the assignment of proofs to proving contexts is balanced over any window of
// consecutive proofs, for every depth the library accepts, and the default depth follows the hardware-queue count.
#include <stdio.h>
#include <stddef.h>
#include <vector>
#include "inflight.h"

using p25::ctx_for_proof;

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (fails++ < 20) {                    \
        printf("FAIL %s: ", #cond);          \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

// per-context loads of the window [start, start + N)
static void loads(size_t start, size_t N, size_t K, size_t& lo, size_t& hi) {
  std::vector<size_t> cnt(K, 0);
  for (size_t i = 0; i < N; i++) {
    const size_t k = ctx_for_proof(start + i, K);
    if (k >= K) {
      CHECK(k < K, "context %zu of %zu", k, K);
      return;
    }
    cnt[k]++;
  }
  lo = hi = cnt[0];
  for (size_t c : cnt) {
    if (c < lo) lo = c;
    if (c > hi) hi = c;
  }
}

int main() {
  // what the prover did before: the in-pass index, restarting at 0 in every witness pass of 64 proofs
  {
    const size_t K = 24;
    std::vector<size_t> cnt(K, 0);
    for (size_t pass = 0; pass < 4; pass++)
      for (size_t p = 0; p < 64; p++) cnt[p % K]++;
    CHECK(cnt[0] == 12 && cnt[15] == 12 && cnt[16] == 8 && cnt[23] == 8, "the defect: %zu %zu", cnt[0], cnt[23]);
  }
  const size_t windows[] = {1, 2, 5, 23, 24, 25, 63, 64, 65, 130, 256};
  for (size_t K = 1; K <= 32; K++)
    for (size_t counter = 0; counter <= 10000; counter++)
      for (size_t N : windows) {
        size_t lo = 0, hi = 0;
        loads(counter, N, K, lo, hi);
        CHECK(hi - lo <= 1, "K %zu counter %zu window %zu: loads %zu..%zu", K, counter, N, lo, hi);
        CHECK(lo == N / K && hi == (N + K - 1) / K, "K %zu counter %zu window %zu: loads %zu..%zu", K, counter, N, lo, hi);
        if (K == 24 && N == 256) CHECK(lo == 10 && hi == 11, "counter %zu: %zu..%zu", counter, lo, hi);
      }
  // a pass's first min(K, bsz) proofs land on different contexts: that is where the prover issues the witness-event waits
  for (size_t K = 1; K <= 32; K++)
    for (size_t counter = 0; counter <= 10000; counter += 7) {
      std::vector<int> seen(K, 0);
      for (size_t p = 0; p < K; p++) seen[ctx_for_proof(counter + p, K)]++;
      for (size_t k = 0; k < K; k++) CHECK(seen[k] == 1, "K %zu counter %zu context %zu seen %d", K, counter, k, seen[k]);
    }
  // the default depth: 16 at the library's own queue settings (and where the count is unknown), deeper from four queues on
  for (int q = 0; q <= 3; q++) CHECK(p25::default_inflight(q) == 16, "queues %d", q);
  for (int q = 4; q <= 32; q++)
    CHECK(p25::default_inflight(q) == p25::INFLIGHT_WIDE_QUEUES && p25::default_inflight(q) >= 16 &&
              p25::default_inflight(q) <= p25::INFLIGHT_MAX,
          "queues %d", q);
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("INFLIGHT OK\n");
  return 0;
}
