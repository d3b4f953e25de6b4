// Stand-alone check of dev_res.h against a counting test double of the HIP runtime (tests/native/fake_hip): every owner
// releases what it holds exactly once, moves transfer ownership and leave the source empty, regrow frees before it
// allocates, and a constructor that throws half way -- at every creation in turn -- gives everything back.  No GPU, no HIP.
#include <stdio.h>
#include <memory>
#include <utility>
#include <vector>
#include "dev_res.h"

using p25::DevEvent;
using p25::DevMem;
using p25::DevStream;
using p25::HipError;

static int fails = 0;
#define CHECK(cond)                                   \
  do {                                                \
    if (!(cond) && fails++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

static FakeHip& F = g_fake_hip;
// every block ends with nothing live and nothing released twice
static void settled() {
  CHECK(F.live() == 0);
  CHECK(F.bad_releases == 0);
  F.calls.clear();
  F.arm(0);
}
template <class Fn>
static bool throws_hip_error(Fn&& fn) {
  try {
    fn();
  } catch (const HipError&) {
    return true;
  }
  return false;
}

// the shape of a proving context: 5 buffers and 3 events, made in the constructor's body
struct Working {
  DevMem a, b, c, d, e;
  DevEvent x, y, z;
  Working() {
    a = DevMem(1);
    b = DevMem(2);
    x.create(hipEventDisableTiming);
    c = DevMem(3);
    d = DevMem(4);
    e = DevMem(5);
    y.create();
    z.create();
  }
};

static void test_mem() {
  {
    DevMem none, zero(0);
    CHECK(!none.p && !none.words && !zero.p && !zero.words && F.calls.empty());
  }
  CHECK(F.calls.empty());   // and nothing to free
  {
    DevMem m(5);
    CHECK(m.p && m.words == 5 && F.calls == "M" && F.last_malloc_bytes == 40 && F.mem.size() == 1);
  }
  CHECK(F.calls == "MF");
  settled();
  {  // move construction
    DevMem m(3);
    uint64_t* p = m.p;
    DevMem n(std::move(m));
    CHECK(n.p == p && n.words == 3 && !m.p && m.words == 0 && F.calls == "M");
  }
  CHECK(F.calls == "MF");
  settled();
  {  // move assignment frees the target's old block; self-move is harmless
    DevMem m(3), n(4);
    uint64_t* p = m.p;
    n = std::move(m);
    CHECK(n.p == p && n.words == 3 && !m.p && m.words == 0 && F.calls == "MMF" && F.mem.size() == 1);
    DevMem& alias = n;
    n = std::move(alias);
    CHECK(n.p == p && n.words == 3 && F.calls == "MMF");
    m = std::move(n);   // into an empty target
    CHECK(m.p == p && m.words == 3 && !n.p && n.words == 0 && F.calls == "MMF");
  }
  CHECK(F.calls == "MMFF");
  settled();
  {  // regrow: free, then allocate; a failure leaves the object empty and the next call allocates
    DevMem m(2);
    m.regrow(6);
    CHECK(F.calls == "MFM" && m.words == 6 && F.last_malloc_bytes == 48 && F.mem.size() == 1);
    F.arm(1);
    CHECK(throws_hip_error([&] { m.regrow(9); }));
    CHECK(!m.p && m.words == 0 && F.calls == "MFMF" && F.mem.empty());
    m.regrow(9);
    CHECK(m.p && m.words == 9 && F.calls == "MFMFM" && F.last_malloc_bytes == 72);
    DevMem fresh;
    fresh.regrow(1);   // from empty: nothing to free
    CHECK(fresh.words == 1 && F.calls == "MFMFMM");
    fresh.regrow(0);   // to nothing
    CHECK(!fresh.p && fresh.words == 0 && F.calls == "MFMFMMF");
  }
  settled();
  F.arm(1);
  CHECK(throws_hip_error([] { DevMem m(7); }));
  settled();
}

static void test_event() {
  {
    DevEvent none;
    CHECK(!none.e && F.calls.empty());
  }
  CHECK(F.calls.empty());
  {
    DevEvent ev;
    ev.create(hipEventDisableTiming);
    hipEvent_t h = ev;
    CHECK(h && h == ev.e && F.calls == "E" && F.last_flags == hipEventDisableTiming);
    ev.ensure(hipEventDisableTiming);
    ev.ensure(hipEventDisableTiming);
    CHECK(ev.e == h && F.calls == "E");   // ensure on a full owner keeps the event
    DevEvent lazy;
    lazy.ensure();
    lazy.ensure();
    CHECK(lazy.e && F.calls == "EE" && F.last_flags == hipEventDefault && F.events.size() == 2);
    DevEvent moved(std::move(ev));
    CHECK(moved.e == h && !ev.e && F.calls == "EE");
    lazy = std::move(moved);   // destroys lazy's own
    CHECK(lazy.e == h && !moved.e && F.calls == "EEe" && F.events.size() == 1);
    DevEvent& alias = lazy;
    lazy = std::move(alias);
    CHECK(lazy.e == h && F.calls == "EEe");
    lazy.create();   // a second create replaces, and destroys, the first
    CHECK(lazy.e && F.calls == "EEeeE" && F.events.size() == 1);
  }
  CHECK(F.calls == "EEeeEe");
  settled();
  {
    DevEvent ev;
    F.arm(1);
    CHECK(throws_hip_error([&] { ev.ensure(); }));
    CHECK(!ev.e);
    ev.ensure();
    CHECK(ev.e);
  }
  settled();
}

static void test_stream() {
  {
    DevStream none;
    CHECK(!none.s && F.calls.empty());
  }
  CHECK(F.calls.empty());
  {
    DevStream st(hipStreamNonBlocking);
    hipStream_t h = st;
    CHECK(h && h == st.s && F.calls == "S" && F.last_flags == hipStreamNonBlocking);
    DevStream moved(std::move(st));
    CHECK(moved.s == h && !st.s && F.calls == "S");
    DevStream other(hipStreamDefault);
    other = std::move(moved);
    CHECK(other.s == h && !moved.s && F.calls == "SSs" && F.streams.size() == 1);
    DevStream& alias = other;
    other = std::move(alias);
    CHECK(other.s == h && F.calls == "SSs");
    st = std::move(other);   // into an empty target
    CHECK(st.s == h && !other.s && F.calls == "SSs");
  }
  CHECK(F.calls == "SSss");
  settled();
  F.arm(1);
  CHECK(throws_hip_error([] { DevStream st(hipStreamNonBlocking); }));
  settled();
}

static void test_half_built() {
  {
    Working w;
    CHECK(F.mem.size() == 5 && F.events.size() == 3 && w.e.words == 5);
  }
  settled();
  for (size_t nth = 1; nth <= 8; nth++) {
    F.arm(nth);
    CHECK(throws_hip_error([] { Working w; }));
    CHECK(F.creations == nth);
    settled();
  }
  F.arm(9);   // there is no ninth creation
  CHECK(!throws_hip_error([] { Working w; }));
  settled();
  // build, then append: a growth that fails leaves the vector as it was
  {
    std::vector<std::unique_ptr<Working>> v;
    auto grow = [&] {
      std::unique_ptr<Working> w(new Working());
      v.push_back(std::move(w));
    };
    grow();
    grow();
    for (size_t nth = 1; nth <= 8; nth++) {
      F.arm(nth);
      CHECK(throws_hip_error(grow));
      CHECK(v.size() == 2 && F.mem.size() == 10 && F.events.size() == 6);
    }
    F.arm(0);
    grow();
    CHECK(v.size() == 3 && v[2]->e.p && F.mem.size() == 15 && F.events.size() == 9);
  }
  settled();
}

int main() {
  test_mem();
  test_event();
  test_stream();
  test_half_built();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("DEV_RES OK\n");
  return 0;
}
