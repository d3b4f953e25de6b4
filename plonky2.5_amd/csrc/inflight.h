// Proofs in flight: how many, and which proving context takes which proof.  Host-only and free of HIP, so that a plain C++
// program can check it (tests/native/inflight.cpp).
#pragma once
#include <stddef.h>

namespace p25 {

// The depth a circuit proves at when the host set none (p25_circuit_set_streams).  HIP streams sharing a hardware queue run
// in order, so a queue needs several contexts to interleave.  At the library's own request of at most two queues 16 is
// the measured optimum (24 was slower, include/p25.h); at four or more, the setting a host exports, the deeper pipeline
// pays (profiles/r10_inflight_depth.txt).  hw_queues = the count in effect, 0 = unknown.
constexpr int INFLIGHT_DEFAULT = 16;
constexpr int INFLIGHT_WIDE_QUEUES = 32;
constexpr int INFLIGHT_MAX = 32;
inline int default_inflight(int hw_queues) { return hw_queues >= 4 ? INFLIGHT_WIDE_QUEUES : INFLIGHT_DEFAULT; }

// Context of the proof with running number `counter` (per circuit; it continues across witness passes and across calls)
// among K contexts.  Any window of N consecutive proofs loads the contexts with floor(N / K) or ceil(N / K) proofs each;
// indexing with the in-pass number instead gave the first 64 mod K contexts one more proof in EVERY pass of 64, 12
// against 8 per 256 proofs at K = 24, and the streams that ran dry left their hardware queue less to interleave.
inline size_t ctx_for_proof(size_t counter, size_t K) { return K ? counter % K : 0; }

}  // namespace p25
