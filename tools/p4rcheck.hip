// Checks the four-round partial blocks of poseidon_p3r.h on the device, on operands that inputs of `permute` cannot
// produce (inside a permutation the block inputs are pseudo-random):
//   blocks   p3r::four_rounds for each of the five blocks against the same four rounds one at a time in canonical gl::
//            arithmetic (true state = registers + the block's deferred offset), one lane per boundary pattern -- every
//            word 0xFFFFFFFFFFFFFFFF, every half 0xFFFFFFFF under each boundary word 0, uniform p - 1, 2^32 - 1, 2^32, 0
//            -- plus 4,096 SplitMix states;
//   rows     every table row (t4[0..11], t3[0], r2, row 0 of M) with ALL halves it multiplies at 0xFFFFFFFF -- state,
//            the d's, the shared sum and the constant: the accumulators at the bound rows_carry_free() asserts (a block
//            cannot be steered there from outside, its d's are S-box outputs) -- and on random halves, against 128-bit
//            host arithmetic;
//   reduce   p3r::reduce_row on boundary and random operands up to its precondition al + (ah >> 32)(2^32 - 1) < 2^64,
//            against (al + ah 2^32) mod p in 128-bit host arithmetic;
//   shared   p3r::shared_sum against the 128-bit sum of the words.
// Prints one "<name>: N mismatches" line each and "P4RCHECK OK".
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "poseidon.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

using namespace poseidon;
typedef unsigned __int128 u128;
constexpr int N_ROWS = WIDTH + 3;   // t4 rows, t3[0], r2, row 0 of M

__global__ void k_blocks(const u64* in, size_t n, int b, u64* out_fast, u64* out_ref) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  if (i >= n) return;
  u64 s[WIDTH], w[WIDTH];
  for (int k = 0; k < WIDTH; k++) {
    s[k] = in[i * WIDTH + k];
    w[k] = gl::add(gl::canon(s[k]), p3r::TBL.off[b][k]);
  }
  p3r::tbl_ptr tp = (p3r::tbl_ptr)&p3r::TBL;
  asm("" : "+s"(tp));
  p3r::four_rounds(s, tp, tp->kc[b], b == p3r::BLOCKS - 1);
  for (int r = 0; r < 4; r++) {   // one round at a time: S-box on lane 0, MDS, the next round's constants
    u64 y[WIDTH];
    for (int k = 0; k < WIDTH; k++) y[k] = w[k];
    const u64 x = y[0], x2 = gl::mul(x, x), x4 = gl::mul(x2, x2), x3 = gl::mul(x, x2);
    y[0] = gl::mul(x3, x4);
    for (int k = 0; k < WIDTH; k++) {
      u64 acc = RC[WIDTH * (p3r::FIRST_BLOCK + 4 * b + r + 1) + k];
      for (int j = 0; j < WIDTH; j++) acc = gl::add(acc, gl::mul(p3r::mds_entry(k, j), y[j]));
      w[k] = acc;
    }
  }
  for (int k = 0; k < WIDTH; k++) {
    out_fast[i * WIDTH + k] = gl::canon(s[k]);
    out_ref[i * WIDTH + k] = gl::sub(w[k], p3r::TBL.off[b + 1][k]);
  }
#endif
}
// in: per lane 12 state words and 4 extra words (u, d1, d2, d3); kc: the constant every row adds (wave-uniform)
__global__ void k_rows(const u64* in, size_t n, u64 kc, u64* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  if (i >= n) return;
  u32 lo[WIDTH], hi[WIDTH], dlo[4], dhi[4];
  for (int k = 0; k < WIDTH; k++) { lo[k] = (u32)in[i * 16 + k]; hi[k] = (u32)(in[i * 16 + k] >> 32); }
  for (int k = 0; k < 4; k++) { dlo[k] = (u32)in[i * 16 + 12 + k]; dhi[k] = (u32)(in[i * 16 + 12 + k] >> 32); }
  p3r::tbl_ptr tp = (p3r::tbl_ptr)&p3r::TBL;
  asm("" : "+s"(tp));
  const u32 klo = __builtin_amdgcn_readfirstlane((u32)kc), khi = __builtin_amdgcn_readfirstlane((u32)(kc >> 32));
  u64* o = out + i * N_ROWS;
#pragma unroll
  for (int r = 0; r < WIDTH; r++) {
    p3r::Row16 cf;
    p3r::load_row(cf, &tp->t4[r]);
    o[r] = gl::canon(p3r::row<0, 4>(lo, hi, cf, dlo, dhi, klo, khi));
  }
  {
    p3r::Row16 cf;
    p3r::load_row(cf, &tp->t3[0]);
    o[WIDTH] = gl::canon(p3r::row<1, 2>(lo, hi, cf, dlo, dhi, klo, khi));
    p3r::load_row(cf, &tp->r2);
    o[WIDTH + 1] = gl::canon(p3r::row<1, 1>(lo, hi, cf, dlo, dhi, klo, khi));
  }
  o[WIDTH + 2] = gl::canon(p3r::row0_m(lo, hi, klo, khi));
#endif
}
__global__ void k_reduce(const u64* al, const u64* ah, size_t n, u64* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  if (i < n) out[i] = gl::canon(p3r::reduce_row(al[i], ah[i]));
#endif
}
__global__ void k_shared(const u64* in, size_t n, u64* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  if (i >= n) return;
  u32 lo[WIDTH], hi[WIDTH];
  for (int k = 0; k < WIDTH; k++) { lo[k] = (u32)in[i * WIDTH + k]; hi[k] = (u32)(in[i * WIDTH + k] >> 32); }
  out[i] = gl::canon(p3r::shared_sum(lo, hi));
#endif
}

static u64 sm_state = 0x243F6A8885A308D3ull;
static u64 splitmix() {
  u64 z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static const u64 P = gl::P;
static const u64 WORDS[] = {0xFFFFFFFFFFFFFFFFull, P - 1, P, 0xFFFFFFFFull, 0x100000000ull, 0, 1, 0xFFFFFFFF00000000ull, 0xFFFFFFFEull};
constexpr int N_WORDS = sizeof WORDS / sizeof *WORDS;

template <class T>
static T* upload(const std::vector<T>& v) {
  T* d = nullptr;
  if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}
static u64 row_host(const p3r::Row16& cf, const u64* v, const u64* d, int e0, int nextra, u64 k, bool& fits) {
  u128 al = (u32)k, ah = k >> 32;
  for (int j = 0; j < WIDTH; j++) { al += (u128)cf.c[j] * (u32)v[j]; ah += (u128)cf.c[j] * (v[j] >> 32); }
  for (int e = e0; e < e0 + nextra; e++) { al += (u128)cf.c[12 + e] * (u32)d[e]; ah += (u128)cf.c[12 + e] * (d[e] >> 32); }
  fits = fits && (al >> 63) == 0 && (ah >> 63) == 0;
  return (u64)((al % P + ((ah % P) << 32)) % P);
}

int main() {
  int total_bad = 0;
  // ---- blocks
  std::vector<u64> st;
  for (int a = 0; a < N_WORDS; a++)
    for (int a0 = 0; a0 < N_WORDS; a0++)
      for (int k = 0; k < WIDTH; k++) st.push_back(k == 0 ? WORDS[a0] : WORDS[a]);
  for (int i = 0; i < 4096 * WIDTH; i++) st.push_back(splitmix());
  const size_t n = st.size() / WIDTH;
  u64 *d_in = upload(st), *d_a = nullptr, *d_b = nullptr;
  if (!d_in) { printf("upload failed\n"); return 1; }
  CK(hipMalloc(&d_a, st.size() * 8));
  CK(hipMalloc(&d_b, st.size() * 8));
  std::vector<u64> ha(st.size()), hb(st.size());
  for (int b = 0; b < p3r::BLOCKS; b++) {
    k_blocks<<<(unsigned)((n + 63) / 64), 64>>>(d_in, n, b, d_a, d_b);
    CK(hipGetLastError());
    CK(hipMemcpy(ha.data(), d_a, st.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), d_b, st.size() * 8, hipMemcpyDeviceToHost));
    int bad = 0;
    for (size_t i = 0; i < st.size(); i++)
      if (ha[i] != hb[i]) { if (bad < 4) printf("  block %d state %zu word %zu: %016llx != %016llx\n", b, i / WIDTH, i % WIDTH, (unsigned long long)ha[i], (unsigned long long)hb[i]); bad++; }
    printf("four_rounds block %d (%zu states): %d mismatches\n", b, n, bad);
    total_bad += bad;
  }
  // ---- rows: lane 0 all halves at their maximum, then boundary words, then random
  {
    std::vector<u64> in;
    for (int k = 0; k < 16; k++) in.push_back(0xFFFFFFFFFFFFFFFFull);
    for (int a = 0; a < N_WORDS; a++)
      for (int k = 0; k < 16; k++) in.push_back(k < WIDTH ? WORDS[a] : 0xFFFFFFFFFFFFFFFFull);
    for (int i = 0; i < 4096 * 16; i++) in.push_back(splitmix());
    const size_t m = in.size() / 16;
    const u64 kc = 0xFFFFFFFFFFFFFFFFull;   // both constant halves at 0xFFFFFFFF
    u64 *d_r = upload(in), *d_o = nullptr;
    if (!d_r) { printf("upload failed\n"); return 1; }
    CK(hipMalloc(&d_o, m * N_ROWS * 8));
    k_rows<<<(unsigned)((m + 63) / 64), 64>>>(d_r, m, kc, d_o);
    CK(hipGetLastError());
    std::vector<u64> out(m * N_ROWS);
    CK(hipMemcpy(out.data(), d_o, out.size() * 8, hipMemcpyDeviceToHost));
    p3r::Row16 m0{};
    for (int j = 0; j < WIDTH; j++) m0.c[j] = (u32)p3r::mds_entry(0, j);
    int bad = 0;
    bool fits = true;
    for (size_t i = 0; i < m; i++) {
      const u64 *v = &in[i * 16], *d = v + WIDTH;
      for (int r = 0; r < N_ROWS; r++) {
        const u64 want = r < WIDTH       ? row_host(p3r::TBL.t4[r], v, d, 0, 4, kc, fits)
                         : r == WIDTH     ? row_host(p3r::TBL.t3[0], v, d, 1, 2, kc, fits)
                         : r == WIDTH + 1 ? row_host(p3r::TBL.r2, v, d, 1, 1, kc, fits)
                                          : row_host(m0, v, d, 0, 0, kc, fits);
        if (out[i * N_ROWS + r] != want) { if (bad < 4) printf("  rows lane %zu row %d: %016llx != %016llx\n", i, r, (unsigned long long)out[i * N_ROWS + r], (unsigned long long)want); bad++; }
      }
    }
    if (!fits) { printf("  a host accumulator reached 2^63\n"); bad++; }
    printf("table rows at maximal halves (%zu lanes x %d rows): %d mismatches\n", m, N_ROWS, bad);
    total_bad += bad;
  }
  // ---- reduce_row
  {
    const u64 B[] = {0, 1, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x1FFFFFFFFull, 1ull << 58, (1ull << 62) - 1,
                     1ull << 62, 0x7FFFFFFF00000000ull, 0x7FFFFFFEFFFFFFFFull, 0x7FFFFFFF00000001ull, 0x7FFFFFFFFFFFFFFEull, 0x7FFFFFFFFFFFFFFFull,
                     1ull << 63, 0xFFFFFFFF00000000ull, P, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull};
    std::vector<u64> al, ah;
    auto legal = [](u64 l, u64 h) { return (u128)l + (u128)(h >> 32) * 0xFFFFFFFFull < ((u128)1 << 64); };
    for (u64 l : B)
      for (u64 h : B)
        if (legal(l, h)) { al.push_back(l); ah.push_back(h); }
    for (int i = 0; i < 1 << 16; i++) {   // random below 2^63, a quarter with the low word of ah all ones / all zeros
      u64 l = splitmix() >> 1, h = splitmix() >> 1;
      if ((i & 3) == 0) h |= 0xFFFFFFFFull;
      if ((i & 7) == 1) h &= ~0xFFFFFFFFull;
      al.push_back(l); ah.push_back(h);
    }
    const size_t m = al.size();
    u64 *d_l = upload(al), *d_h = upload(ah), *d_o = nullptr;
    if (!d_l || !d_h) { printf("upload failed\n"); return 1; }
    CK(hipMalloc(&d_o, m * 8));
    k_reduce<<<(unsigned)((m + 255) / 256), 256>>>(d_l, d_h, m, d_o);
    CK(hipGetLastError());
    std::vector<u64> out(m);
    CK(hipMemcpy(out.data(), d_o, m * 8, hipMemcpyDeviceToHost));
    int bad = 0;
    for (size_t i = 0; i < m; i++) {
      const u64 want = (u64)((al[i] % P + (((u128)(ah[i] % P)) << 32)) % P);
      if (out[i] != want) { if (bad < 4) printf("  reduce_row(%016llx, %016llx): %016llx != %016llx\n", (unsigned long long)al[i], (unsigned long long)ah[i], (unsigned long long)out[i], (unsigned long long)want); bad++; }
    }
    printf("reduce_row (%zu operand pairs): %d mismatches\n", m, bad);
    total_bad += bad;
  }
  // ---- shared_sum
  {
    u64* d_o = nullptr;
    CK(hipMalloc(&d_o, n * 8));
    k_shared<<<(unsigned)((n + 63) / 64), 64>>>(d_in, n, d_o);
    CK(hipGetLastError());
    std::vector<u64> out(n);
    CK(hipMemcpy(out.data(), d_o, n * 8, hipMemcpyDeviceToHost));
    int bad = 0;
    for (size_t i = 0; i < n; i++) {
      u128 sum = 0;
      for (int k = 0; k < WIDTH; k++) sum += st[i * WIDTH + k];
      if (out[i] != (u64)(sum % P)) bad++;
    }
    printf("shared_sum (%zu states): %d mismatches\n", n, bad);
    total_bad += bad;
  }
  CK(hipDeviceSynchronize());
  if (total_bad) { printf("P4RCHECK FAILED\n"); return 1; }
  printf("P4RCHECK OK\n");
  return 0;
}
