// The tail the host-buffer forms of the batch entry points share (prove_batch, verify_batch, P3ProverDev::prove_host,
// verify_host): the per-proof status words come back behind whatever the caller has enqueued on `st`, the stream drains,
// and the host gets them as the C ABI's int32_t.
#pragma once
#include <vector>
#include "dev_res.h"

namespace p25 {

inline void statuses_to_host(const uint32_t* d_status, size_t n, int32_t* statuses, hipStream_t st) {
  std::vector<uint32_t> hs(n);
  P25_HIP(hipMemcpyAsync(hs.data(), d_status, n * 4, hipMemcpyDeviceToHost, st));
  P25_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++) statuses[i] = (int32_t)hs[i];
}

}  // namespace p25
