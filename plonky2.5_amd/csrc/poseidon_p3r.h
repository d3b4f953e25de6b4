// Poseidon partial rounds in blocks: a three-layer head block, then four rounds at a time (included by poseidon.h;
// the tables and their checks are plain constexpr C++, the block functions are device only).
//
// In a partial round only lane 0 passes through the S-box, so with v the state entering the round
// (constants added), d = sbox(v0) - v0 and m0 = column 0 of the MDS matrix M:
//     v' = M v + d m0 + c'.
// Three layers compose to
//     v3 = M^3 v + d0 (M^2 m0) + d1 (M m0) + d2 m0 + (M^2 c1 + M c2 + c3),
// and the two intermediate S-box inputs need one matrix ROW each:
//     v1[0] = (M v)[0] + d0 m0[0] + c1[0],     v2[0] = (M^2 v)[0] + d0 (M m0)[0] + d1 m0[0] + (M c1 + c2)[0].
// M has entries <= 41, so M^3 has entries < 2^22 and row sums 264^3 < 2^24.2: on 32-bit halves of the
// state every sum fits a 64-bit accumulator (< 2^57), i.e. the same carry-free v_mad_u64_u32
// accumulation as the one-round layer (mds_rc).
//
// FOUR rounds.  M^4 itself does not fit: its worst row times 2^32 - 1 is 1.04 * 2^64 (1.13 with the d terms).  But the circulant is dominated
// by its eigenvalue 256.7 (the next is 63.6), so all 144 entries of M^4 lie within [2^28.41, 2^28.51]:
//     M^4 = 2^28 J + R,     J the all-ones matrix, every entry of R in (0, 2^26.76),
// and (2^28 J) v is ONE value shared by the twelve rows: 2^28 u with u = sum_j v_j.  A four-round block therefore
//   * replaces v0 by sbox(v0) first (d0 is simply absorbed: M (v + d0 e0), no separate term in any row);
//   * takes three single rows -- row 0 of M, of M^2, of M^3 -- for the S-box inputs of its rounds 2, 3, 4;
//   * forms u = sum_j v_j mod p once (24 multiply-adds by 1 and one row reduction) and feeds it to every row as a
//     thirteenth word with coefficient 2^28;
//   * runs twelve rows  R[r] . v + 2^28 u + M^3[r][0] d1 + M^2[r][0] d2 + M[r][0] d3 (+ k):  accumulators < 2^62.6.
// That is 16 words per row (Row16) and (12 + 4) x 2 multiply-adds per output word once per FOUR rounds.  The bounds are
// not a comment: rows_carry_free() below is a static_assert on the coefficient sums, and the emulation that proves
// the tables against the round-by-round definition accumulates the 32-bit halves exactly as the device does and fails
// on any accumulator >= 2^63.  (Upstream's sparse "fast partial rounds" need 64-bit constants, i.e. full modular
// multiplies, and come out no cheaper than the dense layer on this ISA.)
//
// The 22 partial rounds (4..25) are scheduled as
//   * a HEAD block that starts from the S-box outputs y of full round 3: its first "round" is just that
//     round's MDS layer (d0 = 0), followed by partial rounds 4 and 5;
//   * five four-round blocks for rounds 6..25;
// so the MDS layer of full round 3 costs nothing extra and no single round is left over.
// Round constants of words 1..11 are DEFERRED: between the head block and the last block the registers hold
// t = (true state) - o, o a constant vector with o[0] = 0 that each block pushes through its own linear map
// (o' = M^n o + K_n, its word 0 taken out and added to the block's row 0), so that the head and the first four blocks
// add constants to their S-box inputs and to row 0 only, and the last block's twelve constants absorb M^4 o and make
// the state true again.  (Word 0 cannot be deferred: it goes through the S-box.)
// The arithmetic is exact integer arithmetic mod p: results are bit-identical to the round-by-round form.
#pragma once

namespace p3r {

constexpr int BLOCKS = 5;         // four-round blocks: rounds 6 + 4 b .. 9 + 4 b
constexpr int HEAD_ROUND = 3;     // the head block replaces MDS(round 3) + partial rounds 4, 5
constexpr int FIRST_BLOCK = 6;    // first round of block 0
static_assert(HEAD_ROUND == HALF_FULL - 1 && FIRST_BLOCK == HEAD_ROUND + 3 &&
                  FIRST_BLOCK + 4 * BLOCKS == HALF_FULL + N_PARTIAL,
              "partial-round schedule");
constexpr int SHIFT4 = 28;        // M^4 = 2^SHIFT4 J + R

struct Row16 {
  u32 c[16];
};
struct Tables {
  Row16 t3[WIDTH];        // M^3 row r | 0, (M m0)[r], m0[r], 0          (t3[0] is also the third single row of a block)
  Row16 t4[WIDTH];        // R row r   | 2^28, (M^2 m0)[r], (M m0)[r], m0[r]
  Row16 r2;               // row 0 of M^2 | 0, m0[0], 0, 0
  u32 kh[32];             // head block: k1.lo, k1.hi, k2.lo, k2.hi, then K3[r].lo, K3[r].hi (r < 12), padding
  u32 kc[BLOCKS][32];     // per block: k1, k2, k3 (lo, hi each), then K4[r].lo, K4[r].hi (r < 12), padding
  u64 off[BLOCKS + 1][WIDTH];   // the deferred offset o of the state entering block b (off[BLOCKS] = 0: the state
                                // leaving the last block is true); no kernel reads it, the block checkers do
};
struct Powers {
  u64 m[5][WIDTH][WIDTH];  // M^0 .. M^4 as integers (entries < 2^29)
};

constexpr u64 mulmod(u64 a, u64 b) { return (u64)((unsigned __int128)a * b % gl::P); }
constexpr u64 addmod(u64 a, u64 b) { return (u64)(((unsigned __int128)a + b) % gl::P); }
constexpr u64 mds_entry(int r, int j) { return MDS_CIRC[(j - r + WIDTH) % WIDTH] + (r == 0 && j == 0 ? MDS_DIAG0 : 0); }

constexpr Powers make_powers() {
  Powers p{};
  for (int r = 0; r < WIDTH; r++) {
    p.m[0][r][r] = 1;
    for (int j = 0; j < WIDTH; j++) p.m[1][r][j] = mds_entry(r, j);
  }
  for (int e = 2; e <= 4; e++)
    for (int r = 0; r < WIDTH; r++)
      for (int j = 0; j < WIDTH; j++)
        for (int k = 0; k < WIDTH; k++) p.m[e][r][j] += p.m[e - 1][r][k] * p.m[1][k][j];
  return p;
}

// constants of a block of n linear layers that are followed by the constants of rounds r0+1 .. r0+n, given the
// deferred offset o of the state entering it (o[0] == 0); on return o is the offset of the state leaving it.
//   out: k_1 .. k_{n-1} (word 0 of the intermediate states: the S-box inputs), then K_n[r], r < 12 (lo, hi each);
//   rows 1..11 of K_n stay deferred (zero in the table, kept in o) unless `last`.
constexpr void block_constants(u32* out, int r0, int n, const Powers& p, u64 (&o)[WIDTH], bool last) {
  u64 oc[WIDTH] = {};   // the entering offset: o is overwritten row by row in the last pass
  for (int j = 0; j < WIDTH; j++) oc[j] = o[j];
  for (int i = 1; i <= n; i++) {
    for (int r = 0; r < (i < n ? 1 : WIDTH); r++) {
      u64 k = RC[WIDTH * (r0 + i) + r];
      for (int j = 0; j < WIDTH; j++) {
        for (int m = 1; m < i; m++) k = addmod(k, mulmod(p.m[m][r][j], RC[WIDTH * (r0 + i - m) + j]));
        k = addmod(k, mulmod(p.m[i][r][j], oc[j]));
      }
      const int at = 2 * (i - 1) + 2 * r;
      const bool now = i < n || r == 0 || last;
      out[at] = now ? (u32)k : 0;
      out[at + 1] = now ? (u32)(k >> 32) : 0;
      if (i == n) o[r] = now ? 0 : k;
    }
  }
}

constexpr Tables make_tables() {
  Tables t{};
  const Powers p = make_powers();
  // v' = M (v + d e0) + c' = M v + d (M e0): m0 = column 0 of M, M m0 = column 0 of M^2, M^2 m0 = column 0 of M^3
  for (int r = 0; r < WIDTH; r++) {
    for (int j = 0; j < WIDTH; j++) {
      t.t3[r].c[j] = (u32)p.m[3][r][j];
      t.t4[r].c[j] = (u32)(p.m[4][r][j] - ((u64)1 << SHIFT4));
    }
    t.t3[r].c[13] = (u32)p.m[2][r][0];
    t.t3[r].c[14] = (u32)p.m[1][r][0];
    t.t4[r].c[12] = 1u << SHIFT4;
    t.t4[r].c[13] = (u32)p.m[3][r][0];
    t.t4[r].c[14] = (u32)p.m[2][r][0];
    t.t4[r].c[15] = (u32)p.m[1][r][0];
  }
  for (int j = 0; j < WIDTH; j++) t.r2.c[j] = (u32)p.m[2][0][j];
  t.r2.c[13] = (u32)p.m[1][0][0];
  u64 o[WIDTH] = {};   // the deferred offset, in program order: head block, then the four-round blocks
  block_constants(t.kh, HEAD_ROUND, 3, p, o, false);
  for (int b = 0; b < BLOCKS; b++) {
    for (int r = 0; r < WIDTH; r++) t.off[b][r] = o[r];
    block_constants(t.kc[b], FIRST_BLOCK + 4 * b, 4, p, o, b == BLOCKS - 1);
  }
  for (int r = 0; r < WIDTH; r++) t.off[BLOCKS][r] = o[r];
  return t;
}
static constexpr Tables TBL = make_tables();

// ---- the proof, at compile time -----------------------------------------------------------------------------------
// (1) Carry-free: every accumulator the block functions form stays below 2^63 for ANY 32-bit halves -- the sum of a
// row's coefficients (state words, the extra terms it uses, 1 for a constant) times 2^32 - 1.  reduce_row needs
// al + (ah >> 32) (2^32 - 1) < 2^64, which al, ah < 2^63 gives.
constexpr bool fits63(const Row16& cf, int e0, int nextra) {
  u64 sum = 1;   // the constant half
  for (int j = 0; j < WIDTH; j++) sum += cf.c[j];
  for (int e = e0; e < e0 + nextra; e++) sum += cf.c[12 + e];
  return (unsigned __int128)sum * 0xFFFFFFFFu < ((unsigned __int128)1 << 63);
}
constexpr bool rows_carry_free() {
  const Powers p = make_powers();
  Row16 m0{};   // row 0 of M, as row0_m has it
  for (int j = 0; j < WIDTH; j++) m0.c[j] = (u32)mds_entry(0, j);
  bool ok = fits63(m0, 0, 0) && fits63(TBL.r2, 1, 1);
  for (int r = 0; r < WIDTH; r++) {
    ok = ok && fits63(TBL.t3[r], 1, 2) && fits63(TBL.t4[r], 0, 4);
    for (int j = 0; j < WIDTH; j++)   // R = M^4 - 2^28 J has non-negative 32-bit entries
      ok = ok && p.m[4][r][j] >= ((u64)1 << SHIFT4) && p.m[4][r][j] - ((u64)1 << SHIFT4) <= 0xFFFFFFFFu;
  }
  return ok;   // (the shared sum u: twelve terms with coefficient 1)
}
static_assert(rows_carry_free(), "poseidon_p3r.h: a row accumulator can reach 2^63");

// (2) The algebra: every block through the tables == the same rounds one at a time.  The emulation splits the words
// into 32-bit halves and accumulates them as the device does (it accepts any u64 representatives and reports an
// accumulator that reaches 2^63); the reference is plain modular arithmetic.
constexpr u64 sbox_ref(u64 x) {
  u64 x2 = mulmod(x, x), x4 = mulmod(x2, x2), x3 = mulmod(x, x2);
  return mulmod(x3, x4);
}
constexpr u64 kpair(const u32* k, int i) { return (u64)k[i] | ((u64)k[i + 1] << 32); }
// reference: `n` rounds starting at round r0 (state has RC[r0] added); skip_first: the first round has no S-box
constexpr void rounds_ref(u64 (&w)[WIDTH], int r0, int n, bool skip_first) {
  for (int k = 0; k < n; k++) {
    u64 y[WIDTH] = {};
    for (int i = 0; i < WIDTH; i++) y[i] = w[i];
    if (!(skip_first && k == 0)) y[0] = sbox_ref(y[0]);
    for (int r = 0; r < WIDTH; r++) {
      u64 acc = RC[WIDTH * (r0 + k + 1) + r];
      for (int j = 0; j < WIDTH; j++) acc = addmod(acc, mulmod(mds_entry(r, j), y[j]));
      w[r] = acc;
    }
  }
}
// al + ah * 2^32 mod p from accumulators of 32-bit halves: what reduce_row computes
constexpr u64 halves_value(unsigned __int128 al, unsigned __int128 ah) {
  return (u64)((al % gl::P + (ah % gl::P << 32)) % gl::P);
}
// one row as row<E0, NEXTRA, WITH_K> forms it; false if an accumulator reaches 2^63
constexpr bool row_emulated(u64& out, const u64 (&v)[WIDTH], const Row16& cf, const u64 (&d)[4], int e0, int nextra,
                            u64 k) {
  unsigned __int128 al = (u32)k, ah = k >> 32;
  for (int j = 0; j < WIDTH; j++) {
    al += (unsigned __int128)cf.c[j] * (u32)v[j];
    ah += (unsigned __int128)cf.c[j] * (v[j] >> 32);
  }
  for (int e = e0; e < e0 + nextra; e++) {
    al += (unsigned __int128)cf.c[12 + e] * (u32)d[e];
    ah += (unsigned __int128)cf.c[12 + e] * (d[e] >> 32);
  }
  out = halves_value(al, ah);
  return (al >> 63) == 0 && (ah >> 63) == 0;
}
constexpr u64 delta_ref(u64 x) { return addmod(sbox_ref(x), gl::P - x % gl::P); }
// the head block (head_block) and a four-round block (four_rounds) through the tables, step for step
constexpr bool block_emulated(u64 (&v)[WIDTH], const u32* kc, bool four, bool last) {
  Row16 m0{};
  for (int j = 0; j < WIDTH; j++) m0.c[j] = (u32)mds_entry(0, j);
  u64 d[4] = {};
  u64 x = 0;
  bool ok = true;
  if (four) v[0] = sbox_ref(v[0]);
  ok = row_emulated(x, v, m0, d, 0, 0, kpair(kc, 0)) && ok;
  d[1] = delta_ref(x);
  ok = row_emulated(x, v, TBL.r2, d, 1, 1, kpair(kc, 2)) && ok;
  d[2] = delta_ref(x);
  if (four) {
    ok = row_emulated(x, v, TBL.t3[0], d, 1, 2, kpair(kc, 4)) && ok;
    d[3] = delta_ref(x);
    unsigned __int128 ul = 0, uh = 0;
    for (int j = 0; j < WIDTH; j++) {
      ul += (u32)v[j];
      uh += v[j] >> 32;
    }
    d[0] = halves_value(ul, uh);
  }
  u64 w[WIDTH] = {};
  for (int r = 0; r < WIDTH; r++) {
    const u64 k = (r == 0 || last) ? kpair(kc, (four ? 6 : 4) + 2 * r) : 0;   // rows 1..11: deferred
    ok = (four ? row_emulated(w[r], v, TBL.t4[r], d, 0, 4, k) : row_emulated(w[r], v, TBL.t3[r], d, 1, 2, k)) && ok;
  }
  for (int r = 0; r < WIDTH; r++) v[r] = w[r];
  return ok;
}
// the whole chain: MDS of round 3 + the 22 partial rounds, from the S-box outputs of round 3 to the state entering
// round 26 (any u64 in, canonical out)
constexpr void chain_ref(u64 (&w)[WIDTH]) {
  for (int i = 0; i < WIDTH; i++) w[i] %= gl::P;
  rounds_ref(w, HEAD_ROUND, 3, true);
  rounds_ref(w, FIRST_BLOCK, 4 * BLOCKS, false);
}
constexpr bool chain_emulated(u64 (&v)[WIDTH]) {
  bool ok = block_emulated(v, TBL.kh, false, false);
  for (int b = 0; b < BLOCKS; b++) ok = block_emulated(v, TBL.kc[b], true, b == BLOCKS - 1) && ok;
  return ok;
}
constexpr bool chain_consistent(int salt) {
  u64 v[WIDTH] = {}, w[WIDTH] = {};
  for (int i = 0; i < WIDTH; i++) v[i] = w[i] = mulmod(0x9E3779B97F4A7C15ull % gl::P, (u64)(i + 1 + 13 * salt));
  chain_ref(w);
  if (!chain_emulated(v)) return false;
  for (int r = 0; r < WIDTH; r++)
    if (v[r] != w[r]) return false;
  return true;
}
constexpr bool tables_consistent() { return chain_consistent(0) && chain_consistent(7) && chain_consistent(101); }
static_assert(tables_consistent(), "poseidon_p3r.h: block tables disagree with the round-by-round definition");

#if defined(__HIP_DEVICE_COMPILE__)
typedef const Tables __attribute__((address_space(4))) * tbl_ptr;
typedef const u32 __attribute__((address_space(4))) * k_ptr;

__device__ __forceinline__ void mad_s(u64& acc, u32 x, u32 coef_sgpr) {
  u64 dm;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=s"(dm) : "v"(x), "s"(coef_sgpr));
}
__device__ __forceinline__ u64 mul_s(u32 x, u32 coef_sgpr) {
  u64 acc, dm;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(acc), "=s"(dm) : "v"(x), "s"(coef_sgpr));
  return acc;
}
template <int C>
__device__ __forceinline__ u64 mul_k(u32 x) {   // x * C, C an inline constant
  u64 acc, dm;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(acc), "=s"(dm) : "v"(x), "n"(C));
  return acc;
}
__device__ __forceinline__ void add_s(u64& acc, u32 k_sgpr) {  // acc += k (a zero-extended 32-bit constant)
  u64 dm;
  asm("v_mad_u64_u32 %0, %1, 1, %2, %0" : "+v"(acc), "=s"(dm) : "s"(k_sgpr));
}
// al + ah * 2^32 mod p (non-canonical result) for al + (ah >> 32) (2^32 - 1) < 2^64 -- in particular for
// al, ah < 2^63; same sequence as in mds_rc.  With ah = ahh 2^32 + ahl the value is
//     X + ahl 2^32,  X = al + ahh (2^32 - 1)        (2^64 == 2^32 - 1 mod p; X < 2^64 is the precondition).
// Adding ahl to the high word x1 of X may carry out of bit 64.  The carry is worth 2^32 - 1, i.e. + 2^32 and - 1: the low word
// loses 1 and, unless that borrows, the high word gains 1 (if it borrows, the borrow and the gain cancel).  No second
// wrap: after a carry the high word is x1 + ahl - 2^32 <= (2^32 - 1) + (2^32 - 1) - 2^32 = 2^32 - 2, so the + 1 cannot
// carry again -- for every x1 and ahl, which is why the bound on al and ah is only the one X needs.
__device__ __forceinline__ u64 reduce_row(u64 al, u64 ah) {
  u32 ahl = (u32)ah, ahh = (u32)(ah >> 32);
  u64 X, dm, t;
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(X), "=s"(dm) : "v"(ahh), "v"(al));
  u32 x0 = (u32)X, x1 = (u32)(X >> 32);
  asm("v_add_co_u32_e32 %1, vcc, %1, %3\n\ts_nop 1\n\t"
      "v_subbrev_co_u32_e64 %0, %2, 0, %0, vcc\n\t"
      "s_andn2_b64 %2, vcc, %2\n\t"
      "v_addc_co_u32_e64 %1, %2, 0, %1, %2"
      : "+v"(x0), "+v"(x1), "=&s"(t)
      : "v"(ahl)
      : "vcc", "scc");
  return gl::make64(x0, x1);
}

// One row: sum_j coef[j] v_j + sum_{e in [E0, E0 + NEXTRA)} coef[12 + e] d_e + k, on 32-bit halves.
template <int E0, int NEXTRA, bool WITH_K = true>
__device__ __forceinline__ u64 row(const u32* lo, const u32* hi, const Row16& cf, const u32* dlo, const u32* dhi,
                                   u32 klo, u32 khi) {
  u64 al = mul_s(lo[0], cf.c[0]), ah = mul_s(hi[0], cf.c[0]);
#pragma unroll
  for (int j = 1; j < WIDTH; j++) {
    mad_s(al, lo[j], cf.c[j]);
    mad_s(ah, hi[j], cf.c[j]);
  }
#pragma unroll
  for (int e = E0; e < E0 + NEXTRA; e++) {
    mad_s(al, dlo[e], cf.c[12 + e]);
    mad_s(ah, dhi[e], cf.c[12 + e]);
  }
  if (WITH_K) {
    add_s(al, klo);
    add_s(ah, khi);
  }
  return reduce_row(al, ah);
}
// Row 0 of M (inline-constant entries 25, 15, 41, ..., 20) applied to the state, + k
__device__ __forceinline__ u64 row0_m(const u32* lo, const u32* hi, u32 klo, u32 khi) {
  u64 al = mul_k<25>(lo[0]), ah = mul_k<25>(hi[0]);
  mad_k<15>(al, lo[1]);  mad_k<15>(ah, hi[1]);
  mad_k<41>(al, lo[2]);  mad_k<41>(ah, hi[2]);
  mad_k<16>(al, lo[3]);  mad_k<16>(ah, hi[3]);
  mad_k<2>(al, lo[4]);   mad_k<2>(ah, hi[4]);
  mad_k<28>(al, lo[5]);  mad_k<28>(ah, hi[5]);
  mad_k<13>(al, lo[6]);  mad_k<13>(ah, hi[6]);
  mad_k<13>(al, lo[7]);  mad_k<13>(ah, hi[7]);
  mad_k<39>(al, lo[8]);  mad_k<39>(ah, hi[8]);
  mad_k<18>(al, lo[9]);  mad_k<18>(ah, hi[9]);
  mad_k<34>(al, lo[10]); mad_k<34>(ah, hi[10]);
  mad_k<20>(al, lo[11]); mad_k<20>(ah, hi[11]);
  add_s(al, klo);
  add_s(ah, khi);
  return reduce_row(al, ah);
}
// u = sum_j v_j mod p (any u64): the word every row of a four-round block takes with coefficient 2^28
__device__ __forceinline__ u64 shared_sum(const u32* lo, const u32* hi) {
  u64 al = mul_k<1>(lo[0]), ah = mul_k<1>(hi[0]);
#pragma unroll
  for (int j = 1; j < WIDTH; j++) {
    mad_k<1>(al, lo[j]);
    mad_k<1>(ah, hi[j]);
  }
  return reduce_row(al, ah);
}
__device__ __forceinline__ void load_row(Row16& cf, const Row16 __attribute__((address_space(4))) * src) {
#pragma unroll
  for (int j = 0; j < 16; j++) cf.c[j] = src->c[j];
}
// d = sbox(x) - x for ANY u64 x (the row reduction's output as it is): the lazy subtraction of gl_lazy.h, both borrows
// corrected, 6 VALU -- the canonical form (gl::canon of x, then gl::sub) cost 10 per partial round.
__device__ __forceinline__ void delta(u64 x, u32& dlo, u32& dhi) {
  const u64 d = gl::sub_nc(sbox(x), x);
  dlo = (u32)d;
  dhi = (u32)(d >> 32);
}
__device__ __forceinline__ void split(const u64 s[WIDTH], u32 lo[WIDTH], u32 hi[WIDTH]) {
#pragma unroll
  for (int i = 0; i < WIDTH; i++) {
    lo[i] = (u32)s[i];
    hi[i] = (u32)(s[i] >> 32);
  }
}

// The head block: s = S-box outputs of the last leading full round; the first layer is that round's MDS, then two
// partial rounds.  On return the state entering round FIRST_BLOCK (minus the deferred offset).
__device__ __forceinline__ void head_block(u64 s[WIDTH], tbl_ptr tp, k_ptr kc) {
  u32 lo[WIDTH], hi[WIDTH];
  split(s, lo, hi);
  u32 dlo[3], dhi[3];   // index = layer whose S-box it is; [0] does not exist
  u64 x = row0_m(lo, hi, kc[0], kc[1]);
  delta(x, dlo[1], dhi[1]);
  {
    Row16 cf;
    load_row(cf, &tp->r2);
    x = row<1, 1>(lo, hi, cf, dlo, dhi, kc[2], kc[3]);
  }
  delta(x, dlo[2], dhi[2]);
#pragma unroll
  for (int r = 0; r < WIDTH; r++) {
    Row16 cf;
    load_row(cf, &tp->t3[r]);
    if (r == 0)
      s[r] = row<1, 2, true>(lo, hi, cf, dlo, dhi, kc[4], kc[5]);
    else   // constants of words 1..11 are deferred to the last block
      s[r] = row<1, 2, false>(lo, hi, cf, dlo, dhi, 0, 0);
  }
}
// Four partial rounds: s = state entering the first of them (constants added, minus the deferred offset); on return
// the state four rounds later.  last (wave-uniform): every row takes its constant, and the state is the true one
// again.  A run-time flag and not a template parameter on purpose: with the last block as a second instance behind
// the loop, the compiler keeps the table rows the loop read alive for it in SGPRs it does not have (some 200
// v_writelane / v_readlane pairs per permutation) and the leaf sponge spills; one loop body with a scalar branch per
// row fits 78 VGPRs without scratch.
__device__ __forceinline__ void four_rounds(u64 s[WIDTH], tbl_ptr tp, k_ptr kc, bool last) {
  s[0] = sbox(s[0]);   // v + d0 e0: the first S-box needs no term of its own
  u32 lo[WIDTH], hi[WIDTH];
  split(s, lo, hi);
  u32 dlo[4], dhi[4];   // [1..3]: d of the block's rounds 2..4; [0]: the shared sum u (coefficient 2^28)
  u64 x = row0_m(lo, hi, kc[0], kc[1]);
  delta(x, dlo[1], dhi[1]);
  {
    Row16 cf;
    load_row(cf, &tp->r2);
    x = row<1, 1>(lo, hi, cf, dlo, dhi, kc[2], kc[3]);
  }
  delta(x, dlo[2], dhi[2]);
  {
    Row16 cf;
    load_row(cf, &tp->t3[0]);
    x = row<1, 2>(lo, hi, cf, dlo, dhi, kc[4], kc[5]);
  }
  delta(x, dlo[3], dhi[3]);
  {
    const u64 u = shared_sum(lo, hi);
    dlo[0] = (u32)u;
    dhi[0] = (u32)(u >> 32);
  }
#pragma unroll
  for (int r = 0; r < WIDTH; r++) {
    Row16 cf;
    load_row(cf, &tp->t4[r]);
    if (r == 0 || last)
      s[r] = row<0, 4, true>(lo, hi, cf, dlo, dhi, kc[6 + 2 * r], kc[7 + 2 * r]);
    else   // constants of words 1..11 are deferred to the last block
      s[r] = row<0, 4, false>(lo, hi, cf, dlo, dhi, 0, 0);
  }
}
// MDS of full round 3 and the 22 partial rounds: s = S-box outputs of round 3 in, the state entering round 26 out
__device__ __forceinline__ void partial_rounds(u64 s[WIDTH]) {
  tbl_ptr tp = (tbl_ptr)&TBL;
  asm("" : "+s"(tp));
  head_block(s, tp, tp->kh);
  for (int b = 0; b < BLOCKS; b++) four_rounds(s, tp, tp->kc[b], b == BLOCKS - 1);
}
#endif

}  // namespace p3r
