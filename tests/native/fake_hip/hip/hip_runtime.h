// Test double for the HIP runtime, as far as plonky2.5_amd/csrc/dev_res.h calls it (tests/native/dev_res.cpp; the precedent
// is tests/c_abi/fake_rccl.cpp).  It counts the live objects of each kind, keeps the order of the calls, and fails the N-th
// creation (of any kind, counted from arming) on request.  Header-only; no GPU, no HIP.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <map>
#include <set>
#include <string>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct fake_hip_event* hipEvent_t;
typedef struct fake_hip_stream* hipStream_t;
enum : unsigned { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamDefault = 0, hipStreamNonBlocking = 1 };

struct FakeHip {
  std::set<void*> mem, events, streams;   // live objects
  std::string calls;                      // M malloc, F free, E / e event create / destroy, S / s stream create / destroy
  size_t last_malloc_bytes = 0, creations = 0, fail_at = 0, bad_releases = 0;
  unsigned last_flags = 0;
  size_t bytes_requested = 0, bytes_live = 0;   // running totals over the hipMallocs that succeeded / that are not freed yet
  std::map<void*, size_t> bytes_of;             // ... per live block
  void arm(size_t nth) {   // the nth creation from now fails (0: none does)
    creations = 0;
    fail_at = nth;
  }
  bool fails() { return ++creations == fail_at; }
  size_t live() const { return mem.size() + events.size() + streams.size(); }
  // a released handle must be live: a double or stray release is counted, not performed
  void release(std::set<void*>& live_set, void* h, char tag) {
    calls += tag;
    if (!live_set.erase(h)) {
      bad_releases++;
      return;
    }
    free(h);
  }
};
inline FakeHip g_fake_hip;

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake failure"; }
template <class T>
inline hipError_t hipMalloc(T** p, size_t bytes) {
  if (g_fake_hip.fails()) return hipErrorOutOfMemory;
  g_fake_hip.calls += 'M';
  g_fake_hip.last_malloc_bytes = bytes;
  *p = (T*)malloc(bytes ? bytes : 1);
  g_fake_hip.mem.insert(*p);
  g_fake_hip.bytes_requested += bytes;
  g_fake_hip.bytes_live += bytes;
  g_fake_hip.bytes_of[*p] = bytes;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  auto it = g_fake_hip.bytes_of.find(p);
  if (it != g_fake_hip.bytes_of.end()) {
    g_fake_hip.bytes_live -= it->second;
    g_fake_hip.bytes_of.erase(it);
  }
  g_fake_hip.release(g_fake_hip.mem, p, 'F');
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (g_fake_hip.fails()) return hipErrorOutOfMemory;
  g_fake_hip.calls += 'E';
  g_fake_hip.last_flags = flags;
  *e = (hipEvent_t)malloc(1);
  g_fake_hip.events.insert(*e);
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  g_fake_hip.release(g_fake_hip.events, e, 'e');
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
  if (g_fake_hip.fails()) return hipErrorOutOfMemory;
  g_fake_hip.calls += 'S';
  g_fake_hip.last_flags = flags;
  *s = (hipStream_t)malloc(1);
  g_fake_hip.streams.insert(*s);
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  g_fake_hip.release(g_fake_hip.streams, s, 's');
  return hipSuccess;
}
