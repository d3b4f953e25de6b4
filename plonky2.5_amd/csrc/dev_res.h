// Owners of the library's device resources: every hipMalloc, event and stream the library frees has exactly one of these
// as its owner, so a constructor that throws half way, or an exception between a creation and its release, leaks nothing.
// Move-only; a moved-from or default-constructed owner is empty.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace p25 {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
#define P25_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw p25::HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " at " +        \
                          __FILE__ + ":" + std::to_string(__LINE__));                         \
  } while (0)

struct DevMem {  // owning device allocation of `words` 64-bit words
  uint64_t* p = nullptr;
  size_t words = 0;
  DevMem() {}
  explicit DevMem(size_t w) { alloc(w); }
  ~DevMem() { release(); }
  DevMem(DevMem&& o) noexcept : p(o.p), words(o.words) {
    o.p = nullptr;
    o.words = 0;
  }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      words = o.words;
      o.p = nullptr;
      o.words = 0;
    }
    return *this;
  }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  // Frees the old block FIRST, then allocates: the two never coexist, so a buffer can grow to more than half of what is
  // free.  After a failure the object is empty (words == 0) and the next call allocates again.  The caller sees to it
  // that nothing in flight still reads the old block.
  void regrow(size_t w) {
    release();
    alloc(w);
  }

 private:
  void alloc(size_t w) {
    if (w) P25_HIP(hipMalloc(&p, w * sizeof(uint64_t)));
    words = w;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    words = 0;
  }
};

struct DevEvent {  // owns one hipEvent_t; empty until create / ensure
  hipEvent_t e = nullptr;
  DevEvent() {}
  ~DevEvent() { release(); }
  DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) {
      release();
      e = o.e;
      o.e = nullptr;
    }
    return *this;
  }
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  void create(unsigned flags = hipEventDefault) {
    release();
    P25_HIP(hipEventCreateWithFlags(&e, flags));
  }
  void ensure(unsigned flags = hipEventDefault) {
    if (!e) create(flags);
  }
  operator hipEvent_t() const { return e; }

 private:
  void release() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
};

struct DevStream {  // owns one stream created with the given flags; empty by default
  hipStream_t s = nullptr;
  DevStream() {}
  explicit DevStream(unsigned flags) { P25_HIP(hipStreamCreateWithFlags(&s, flags)); }
  ~DevStream() { release(); }
  DevStream(DevStream&& o) noexcept : s(o.s) { o.s = nullptr; }
  DevStream& operator=(DevStream&& o) noexcept {
    if (this != &o) {
      release();
      s = o.s;
      o.s = nullptr;
    }
    return *this;
  }
  DevStream(const DevStream&) = delete;
  DevStream& operator=(const DevStream&) = delete;
  operator hipStream_t() const { return s; }

 private:
  void release() {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  }
};

}  // namespace p25
