// Index maps of k_ntt_tile (kernels_ntt.hip): where lane `tid` of a block finds its k-th element in global memory and in
// the LDS tile, for each addressing form the library issues.  Free of HIP when a host compiler reads it, so that a plain
// C++ program can check the maps against their closed forms (tests/native/ntt_index.cpp).
//
// A block of `nth` lanes owns a tile of T = 2^log_t sub-transforms of R = 2^log_r points, tg0 = tile * T the first of them;
// NT = 2^log_nt sub-transforms make a polynomial.  Lane tid handles the elements e = tid + k * nth, e < T * R.  nth is a
// multiple of T, so in the t-contiguous kinds a lane's t never changes and its i advances by nth / T: every quantity is
// an add away from its predecessor.  In the i-contiguous kinds the global offset is tile base + e.  All offsets are in
// words inside one polynomial (one coset of it in pass 1 of an LDE, all 2^rate_bits cosets in its pass 2) and fit 32
// bits: a polynomial has at most 2^25 words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NTTIX_HD __host__ __device__ __forceinline__
#else
#define NTTIX_HD inline
#endif

namespace p25 {
namespace nttix {

// Input: element (t, i) of the tile is read from
enum In : int {
  IN_T = 0,     // t-contiguous:  (tg0 + t) + i * NT
  IN_I = 1,     // i-contiguous:  (tg0 + t) * R + i
  IN_I_BR = 2,  // i-contiguous, row and position bit-reversed:  rev(tg0 + t) * R + rev(i)
};
// Output: LDS position q of sub-transform t holds frequency j = rev(q) (the DIF network leaves bit-reversed order) and goes to
enum Out : int {
  OUT_T = 0,     // t-contiguous, natural:        (tg0 + t) + j * NT
  OUT_T_BR = 1,  // t-contiguous, rows reversed:  (tg0 + t) + q * NT
  OUT_I = 2,     // i-contiguous, natural:        (tg0 + t) * R + j
  OUT_I_BR = 3,  // i-contiguous, reversed:       (tg0 + t) * R + q
};
// What the store phase multiplies output (t, j) by
enum Mul : int {
  MUL_NONE = 0,
  MUL_TWIDDLE = 1,  // the four-step twiddle pow_table[(tg0 + t) * j]
  MUL_POST = 2,     // the inverse's post-scale post_t[tg0 + t] * post_i[j]
};

struct Tile {
  int log_r, log_t, log_nt;
  uint32_t tg0;
};

NTTIX_HD uint32_t brev(uint32_t x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
  uint32_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((x >> b) & 1u) << (bits - 1 - b);
  return r;
#endif
}
// words per LDS row of the tile: T, padded by one so that both access directions are conflict-free
NTTIX_HD uint32_t row_pitch(int log_t) { return log_t ? (1u << log_t) + 1u : 1u; }

// Block L of a launch -> (tile, polynomial, coset): the low log_g bits of L pick the tile's residue (the XCD), the cosets of
// one tile follow each other, then the other tiles of the residue class, then the polynomials.
struct BlockId {
  uint32_t tile, poly, coset;
};
NTTIX_HD BlockId decode_block(uint32_t L, uint32_t log_g, uint32_t n_tiles, uint32_t n_cosets) {
  const uint32_t m = L >> log_g, tiles_g = n_tiles >> log_g;
  const uint32_t r = m / n_cosets;
  return BlockId{(r % tiles_g) * (1u << log_g) + (L & ((1u << log_g) - 1u)), r / tiles_g, m % n_cosets};
}

// Coset c of an LDE over 2^log_cosets cosets is stored as the block of N words number rev(c): the LDE's bit-reversed order
NTTIX_HD uint32_t coset_block(uint32_t coset, int log_cosets) { return brev(coset, log_cosets); }

// The load phase: global offset, LDS slot and element index i of the lane's current element; next() moves to e + nth.
template <int IN>
struct LoadCursor {
  uint32_t g, s, i;     // IN_T: the three quantities themselves ...
  uint32_t dg, ds, di;  // ... and what nth more elements add to them
  uint32_t e, de, base; // IN_I*: the element number, its advance and the tile's first word
  int log_r, log_nt;
  uint32_t tp, tg0;

  NTTIX_HD void init(const Tile& a, uint32_t tid, uint32_t nth) {
    log_r = a.log_r, log_nt = a.log_nt, tp = row_pitch(a.log_t), tg0 = a.tg0;
    if constexpr (IN == IN_T) {
      const uint32_t t = tid & ((1u << a.log_t) - 1u);
      i = tid >> a.log_t, di = nth >> a.log_t;
      g = tg0 + t + (i << log_nt), dg = di << log_nt;
      s = i * tp + t, ds = di * tp;
    } else {
      e = tid, de = nth, base = tg0 << log_r;
    }
  }
  NTTIX_HD void next() {
    if constexpr (IN == IN_T) g += dg, s += ds, i += di;
    else e += de;
  }
  NTTIX_HD uint32_t idx() const {
    if constexpr (IN == IN_T) return i;
    const uint32_t off = e & ((1u << log_r) - 1u);
    return IN == IN_I_BR ? brev(off, log_r) : off;
  }
  NTTIX_HD uint32_t slot() const {
    if constexpr (IN == IN_T) return s;
    return idx() * tp + (e >> log_r);
  }
  NTTIX_HD uint32_t goff() const {
    if constexpr (IN == IN_T) return g;
    if constexpr (IN == IN_I) return base + e;
    return (brev(tg0 + (e >> log_r), log_nt) << log_r) + (e & ((1u << log_r) - 1u));
  }
};

// The store phase: global offset, LDS slot, and the two factors (tw, j) of the multiplier's index.
template <int OUT>
struct StoreCursor {
  uint32_t g, s, q;     // OUT_T*: offset (OUT_T_BR), slot and LDS position ...
  uint32_t dg, ds, dq;  // ... and what nth more elements add to them
  uint32_t e, de, base; // OUT_I*: the element number, its advance and the tile's first word
  int log_r, log_nt;
  uint32_t tp, tg0, twv;

  NTTIX_HD void init(const Tile& a, uint32_t tid, uint32_t nth) {
    log_r = a.log_r, log_nt = a.log_nt, tp = row_pitch(a.log_t), tg0 = a.tg0;
    if constexpr (OUT == OUT_T || OUT == OUT_T_BR) {
      const uint32_t t = tid & ((1u << a.log_t) - 1u);
      twv = tg0 + t;
      q = tid >> a.log_t, dq = nth >> a.log_t;
      g = twv + (q << log_nt), dg = dq << log_nt;
      s = q * tp + t, ds = dq * tp;
    } else {
      e = tid, de = nth, base = tg0 << log_r;
    }
  }
  NTTIX_HD void next() {
    if constexpr (OUT == OUT_T || OUT == OUT_T_BR) g += dg, s += ds, q += dq;
    else e += de;
  }
  // sub-transform number of the element: the first factor of the twiddle index, the index into post_t
  NTTIX_HD uint32_t tw() const {
    if constexpr (OUT == OUT_T || OUT == OUT_T_BR) return twv;
    return tg0 + (e >> log_r);
  }
  // frequency index of the element: the second factor of the twiddle index, the index into post_i
  NTTIX_HD uint32_t j() const {
    if constexpr (OUT == OUT_T || OUT == OUT_T_BR) return brev(q, log_r);
    const uint32_t off = e & ((1u << log_r) - 1u);
    return OUT == OUT_I_BR ? brev(off, log_r) : off;
  }
  NTTIX_HD uint32_t slot() const {
    if constexpr (OUT == OUT_T || OUT == OUT_T_BR) return s;
    const uint32_t off = e & ((1u << log_r) - 1u);
    return (OUT == OUT_I_BR ? off : brev(off, log_r)) * tp + (e >> log_r);
  }
  NTTIX_HD uint32_t goff() const {
    if constexpr (OUT == OUT_T_BR) return g;
    if constexpr (OUT == OUT_T) return twv + (j() << log_nt);
    return base + e;
  }
};

}  // namespace nttix
}  // namespace p25
