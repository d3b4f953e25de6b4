// CPU check of the partial-round block tables of poseidon_p3r.h: the host emulation of the head block and the five
// four-round blocks (32-bit halves accumulated as the device accumulates them, every accumulator checked against 2^63)
// against the round-by-round definition --
//   * the whole permutation built on the blocks against poseidon::permute on 10^5 random states;
//   * the chain of blocks on states no permutation input can produce (any u64 words, all-ones halves);
//   * every block on its own, with the deferred offset the tables record for it;
//   * the coefficient sums behind "carry-free", recomputed here from M with 128-bit integers.
// Prints "POSEIDON BLOCKS OK".
#include <stdio.h>
#include <stdlib.h>
#include "poseidon.h"

using namespace poseidon;
typedef unsigned __int128 u128;
static const u64 P = gl::P;
static u64 sm_state = 0x0123456789ABCDEFull;
static u64 splitmix() {
  u64 z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad < 10) { printf(__VA_ARGS__); printf("\n"); } bad++; } } while (0)

// full round r (constants of round r already added): S-boxes, MDS, constants of round r + 1 (none after the last)
static void full_round(u64 (&w)[WIDTH], int r) {
  u64 y[WIDTH];
  for (int i = 0; i < WIDTH; i++) y[i] = p3r::sbox_ref(w[i]);
  for (int i = 0; i < WIDTH; i++) {
    u64 acc = r + 1 < N_ROUNDS ? RC[WIDTH * (r + 1) + i] : 0;
    for (int j = 0; j < WIDTH; j++) acc = p3r::addmod(acc, p3r::mulmod(p3r::mds_entry(i, j), y[j]));
    w[i] = acc;
  }
}
// the permutation with the partial rounds taken through the block tables
static bool permute_blocks(u64 (&w)[WIDTH]) {
  for (int i = 0; i < WIDTH; i++) w[i] = p3r::addmod(w[i], RC[i]);
  for (int r = 0; r < HALF_FULL - 1; r++) full_round(w, r);
  for (int i = 0; i < WIDTH; i++) w[i] = p3r::sbox_ref(w[i]);   // round 3's S-boxes; its MDS is the head block's
  const bool ok = p3r::chain_emulated(w);
  for (int r = HALF_FULL + N_PARTIAL; r < N_ROUNDS; r++) full_round(w, r);
  return ok;
}

static void chain_case(const u64 (&in)[WIDTH], const char* what) {
  u64 v[WIDTH], w[WIDTH];
  for (int i = 0; i < WIDTH; i++) v[i] = w[i] = in[i];
  p3r::chain_ref(w);
  CHECK(p3r::chain_emulated(v), "%s: an accumulator reached 2^63", what);
  for (int i = 0; i < WIDTH; i++) CHECK(v[i] == w[i], "%s: word %d %016llx != %016llx", what, i, (unsigned long long)v[i], (unsigned long long)w[i]);
}
// block b alone: registers t = w - off[b] for a true state w entering round 6 + 4 b; afterwards t' + off[b + 1] is the
// state four rounds later
static void block_case(int b, const u64 (&in)[WIDTH], const char* what) {
  u64 t[WIDTH], w[WIDTH];
  for (int i = 0; i < WIDTH; i++) {
    t[i] = in[i];   // any u64
    w[i] = p3r::addmod(in[i], p3r::TBL.off[b][i]);
  }
  p3r::rounds_ref(w, p3r::FIRST_BLOCK + 4 * b, 4, false);
  CHECK(p3r::block_emulated(t, p3r::TBL.kc[b], true, b == p3r::BLOCKS - 1), "%s block %d: an accumulator reached 2^63", what, b);
  for (int i = 0; i < WIDTH; i++)
    CHECK(p3r::addmod(t[i], p3r::TBL.off[b + 1][i]) == w[i], "%s block %d word %d", what, b, i);
}

int main() {
  // (1) 10^5 random canonical states through the whole permutation
  for (int n = 0; n < 100000; n++) {
    u64 a[WIDTH], b[WIDTH];
    for (int i = 0; i < WIDTH; i++) a[i] = b[i] = splitmix() % P;
    permute(a);
    CHECK(permute_blocks(b), "state %d: an accumulator reached 2^63", n);
    for (int i = 0; i < WIDTH; i++) CHECK(a[i] == b[i], "state %d word %d: %016llx != %016llx", n, i, (unsigned long long)a[i], (unsigned long long)b[i]);
  }
  // (2), (3) boundary patterns: the chain and every block
  const u64 words[] = {0xFFFFFFFFFFFFFFFFull, P - 1, P, 0xFFFFFFFFull, 0x100000000ull, 0, 1, 0xFFFFFFFF00000000ull, 0x00000000FFFFFFFEull};
  for (u64 x : words)
    for (u64 x0 : words) {
      u64 s[WIDTH];
      for (int i = 0; i < WIDTH; i++) s[i] = i == 0 ? x0 : x;
      chain_case(s, "uniform words");
      for (int b = 0; b < p3r::BLOCKS; b++) block_case(b, s, "uniform words");
    }
  for (int n = 0; n < 4096; n++) {
    u64 s[WIDTH];
    for (int i = 0; i < WIDTH; i++) {
      const u64 r = splitmix();
      s[i] = (r & 3) == 0 ? words[(r >> 2) % (sizeof words / sizeof *words)] : splitmix();
    }
    chain_case(s, "mixed words");
    block_case(n % p3r::BLOCKS, s, "mixed words");
  }
  // (4) the bounds, from M directly: the worst row of M^4 does NOT fit, the residual rows with everything they carry do
  u128 M[WIDTH][WIDTH], A[WIDTH][WIDTH], B[WIDTH][WIDTH], col[5][WIDTH];
  for (int r = 0; r < WIDTH; r++)
    for (int j = 0; j < WIDTH; j++) { M[r][j] = p3r::mds_entry(r, j); A[r][j] = M[r][j]; }
  for (int r = 0; r < WIDTH; r++) col[1][r] = M[r][0];
  for (int e = 2; e <= 4; e++) {
    for (int r = 0; r < WIDTH; r++)
      for (int j = 0; j < WIDTH; j++) { B[r][j] = 0; for (int k = 0; k < WIDTH; k++) B[r][j] += A[r][k] * M[k][j]; }
    for (int r = 0; r < WIDTH; r++) { col[e][r] = B[r][0]; for (int j = 0; j < WIDTH; j++) A[r][j] = B[r][j]; }
  }
  const u128 half = 0xFFFFFFFFull, lim63 = (u128)1 << 63, lim64 = (u128)1 << 64;
  u128 worst_full = 0, worst_res = 0;
  for (int r = 0; r < WIDTH; r++) {
    u128 full = 0, res = 0;
    for (int j = 0; j < WIDTH; j++) {
      full += A[r][j];
      CHECK(A[r][j] >= ((u128)1 << 28) && A[r][j] - ((u128)1 << 28) == p3r::TBL.t4[r].c[j], "t4[%d][%d]", r, j);
      res += A[r][j] - ((u128)1 << 28);
    }
    res += ((u128)1 << 28) + col[3][r] + col[2][r] + col[1][r] + 1;   // u, d1, d2, d3, a constant half
    CHECK(p3r::TBL.t4[r].c[12] == 1u << 28 && p3r::TBL.t4[r].c[13] == col[3][r] && p3r::TBL.t4[r].c[14] == col[2][r] &&
              p3r::TBL.t4[r].c[15] == col[1][r], "t4[%d] extras", r);
    if (full * half > worst_full) worst_full = full * half;
    if (res * half > worst_res) worst_res = res * half;
  }
  CHECK(worst_full >= lim64, "M^4 was expected to overflow a 64-bit accumulator");
  CHECK(worst_res < lim63, "a residual row can reach 2^63");
  printf("worst row of M^4: %.4f * 2^64; worst residual row with its extras: %.4f * 2^63\n",
         (double)worst_full / 18446744073709551616.0, (double)worst_res / 9223372036854775808.0);
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("POSEIDON BLOCKS OK\n");
  return 0;
}
