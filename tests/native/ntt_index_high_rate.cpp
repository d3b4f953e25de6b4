// Stand-alone check of ntt_index.h at the extremes of the 2^rb-coset LDE (rb up to 8; no GPU, no HIP), in the manner of
// ntt_index.cpp, which covers every form at the shapes up to rate 3.
//
// ntt_lde_bitrev(log_n, rb) with log_n = l1 + l2 (l2 = log_n / 2; a single pass up to 2^10) issues
//   pass 1   IN_T  -> OUT_T_BR, tile (log_r = l2, log_nt = l1), once per coset: 2^rb blocks per coefficient tile; coset c
//            is stored from word coset_block(c, rb) * n on; the twiddle index is tw * j;
//   pass 2   IN_I  -> OUT_I_BR, tile (log_r = l1, log_nt = l2 + rb) over all cosets of a polynomial at once: B = n << rb
//            words, up to 2^24, every offset a uint32_t.
// Checked against closed forms in 64-bit arithmetic: no cursor offset wraps, a launch covers the polynomial exactly once,
// the twiddle product stays inside 24 bits, the cosets' blocks tile the LDE, and a tile's 2^rb blocks run back to back on
// one XCD.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "ntt_index.h"

using namespace p25::nttix;

static int fails = 0;
static long checked = 0;
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

static uint64_t rev(uint64_t x, int bits) {
  uint64_t r = 0;
  for (int b = 0; b < bits; b++)
    if (x >> b & 1) r |= (uint64_t)1 << (bits - 1 - b);
  return r;
}

// the library's split and tile widths (kernels_ntt.hip: split, pick_log_t, tile_lds_bytes), restated
static void split(int log_n, int& l1, int& l2) {
  if (log_n <= 10) {
    l1 = 0, l2 = log_n;
  } else {
    l2 = log_n / 2, l1 = log_n - l2;
  }
}
static size_t tile_lds_bytes(int log_r, int log_t) {
  const size_t R = (size_t)1 << log_r, T = (size_t)1 << log_t, TP = T > 1 ? T + 1 : 1;
  return (R * TP + (log_r <= 10 ? R : R / 2)) * 8;
}
static int pick_log_t(int log_r, int log_nt, bool strided) {
  int lt = 12 - log_r;
  if (strided)
    for (int w = 4; w > lt; w--)
      if (tile_lds_bytes(log_r, w) <= 79 * 1024) {
        lt = w;
        break;
      }
  if (!strided && log_r == 10) lt = 3;
  if (lt > 4) lt = 4;
  if (lt > log_nt) lt = log_nt;
  if (lt < 0) lt = 0;
  return lt;
}

struct Shape {
  int log_r, log_t, log_nt;
  uint32_t nth;
};

// pass 2 (and the single pass): IN_I loads, OUT_I_BR stores, over the whole polynomial
static void check_pass2(const Shape& s) {
  const uint64_t T = 1ull << s.log_t, R = 1ull << s.log_r, NT = 1ull << s.log_nt, TP = T > 1 ? T + 1 : 1, TR = T * R;
  std::vector<uint8_t> in_seen(NT * R, 0), out_seen(NT * R, 0);
  for (uint64_t tile = 0; tile < NT / T; tile++) {
    const Tile tl{s.log_r, s.log_t, s.log_nt, (uint32_t)(tile * T)};
    for (uint32_t tid = 0; tid < s.nth; tid++) {
      LoadCursor<IN_I> lc;
      StoreCursor<OUT_I_BR> sc;
      lc.init(tl, tid, s.nth);
      sc.init(tl, tid, s.nth);
      for (uint64_t e = tid; e < TR; e += s.nth, lc.next(), sc.next()) {
        checked++;
        const uint64_t t = e >> s.log_r, off = e & (R - 1), addr = (tile * T + t) * R + off;   // 64-bit closed form
        CHECK(lc.goff() == addr && lc.idx() == off && lc.slot() == off * TP + t, "load r %d t %d nt %d tile %llu e %llu: (%u, %u, %u)",
              s.log_r, s.log_t, s.log_nt, (unsigned long long)tile, (unsigned long long)e, lc.goff(), lc.idx(), lc.slot());
        // LDS position q = off holds frequency rev(off); OUT_I_BR stores it at word off of the row: bit-reversed order
        CHECK(sc.goff() == addr && sc.slot() == off * TP + t && sc.j() == rev(off, s.log_r) && sc.tw() == tile * T + t,
              "store r %d t %d nt %d tile %llu e %llu: (%u, %u, %u, %u)", s.log_r, s.log_t, s.log_nt, (unsigned long long)tile,
              (unsigned long long)e, sc.goff(), sc.slot(), sc.j(), sc.tw());
        if (addr < NT * R) {
          CHECK(!in_seen[addr]++, "word %llu loaded twice", (unsigned long long)addr);
          CHECK(!out_seen[addr]++, "word %llu stored twice", (unsigned long long)addr);
        }
      }
    }
  }
  size_t a = 0, b = 0;
  for (uint8_t v : in_seen) a += v == 1;
  for (uint8_t v : out_seen) b += v == 1;
  CHECK(a == NT * R && b == NT * R, "pass 2 r %d t %d nt %d: %zu loads, %zu stores of %llu words", s.log_r, s.log_t, s.log_nt, a, b,
        (unsigned long long)(NT * R));
}

// pass 1 of one coset: IN_T loads, OUT_T_BR stores with the four-step twiddle pow_table[tw * j]
static void check_pass1(const Shape& s) {
  const uint64_t T = 1ull << s.log_t, R = 1ull << s.log_r, NT = 1ull << s.log_nt, TP = T > 1 ? T + 1 : 1, TR = T * R;
  std::vector<uint8_t> in_seen(NT * R, 0), out_seen(NT * R, 0);
  for (uint64_t tile = 0; tile < NT / T; tile++) {
    const Tile tl{s.log_r, s.log_t, s.log_nt, (uint32_t)(tile * T)};
    for (uint32_t tid = 0; tid < s.nth; tid++) {
      LoadCursor<IN_T> lc;
      StoreCursor<OUT_T_BR> sc;
      lc.init(tl, tid, s.nth);
      sc.init(tl, tid, s.nth);
      for (uint64_t e = tid; e < TR; e += s.nth, lc.next(), sc.next()) {
        checked++;
        const uint64_t t = e & (T - 1), i = e >> s.log_t, tg = tile * T + t, addr = tg + i * NT;
        CHECK(lc.goff() == addr && lc.idx() == i && lc.slot() == i * TP + t, "load r %d t %d nt %d e %llu", s.log_r, s.log_t, s.log_nt,
              (unsigned long long)e);
        CHECK(sc.goff() == addr && sc.slot() == i * TP + t && sc.j() == rev(i, s.log_r) && sc.tw() == tg, "store r %d t %d nt %d e %llu",
              s.log_r, s.log_t, s.log_nt, (unsigned long long)e);
        // __umul24(tw, j) indexes the power table of n = NT * R entries: both factors and the product inside 24 bits
        CHECK(sc.tw() < (1u << 24) && sc.j() < (1u << 24) && (uint64_t)sc.tw() * sc.j() < NT * R && NT * R <= (1ull << 24),
              "twiddle index %u * %u", sc.tw(), sc.j());
        if (addr < NT * R) {
          CHECK(!in_seen[addr]++, "word %llu loaded twice", (unsigned long long)addr);
          CHECK(!out_seen[addr]++, "word %llu stored twice", (unsigned long long)addr);
        }
      }
    }
  }
  size_t a = 0, b = 0;
  for (uint8_t v : in_seen) a += v == 1;
  for (uint8_t v : out_seen) b += v == 1;
  CHECK(a == NT * R && b == NT * R, "pass 1 r %d t %d nt %d: %zu loads, %zu stores", s.log_r, s.log_t, s.log_nt, a, b);
}

// the launch of pass 1: every (tile, polynomial, coset) once, a tile's cosets back to back on the tile's XCD, and the
// cosets' output blocks a permutation of the 2^rb blocks of n words
static void check_decode(uint32_t log_tiles, int rb, uint32_t n_polys) {
  const uint32_t n_tiles = 1u << log_tiles, n_cosets = 1u << rb;
  uint32_t log_g = 0;
  while (log_g < 3 && (2u << log_g) <= n_tiles) log_g++;
  const uint64_t total = (uint64_t)n_tiles * n_cosets * n_polys;
  CHECK(total < (1ull << 32), "grid of %llu blocks", (unsigned long long)total);
  std::vector<uint8_t> seen(total, 0);
  const uint32_t g = 1u << log_g;
  for (uint64_t L = 0; L < total; L++) {
    const BlockId b = decode_block((uint32_t)L, log_g, n_tiles, n_cosets);
    if (b.tile >= n_tiles || b.poly >= n_polys || b.coset >= n_cosets) {
      CHECK(false, "block %llu: (%u, %u, %u)", (unsigned long long)L, b.tile, b.poly, b.coset);
      continue;
    }
    CHECK((b.tile & (g - 1)) == (L & (g - 1)), "block %llu: tile %u on another XCD", (unsigned long long)L, b.tile);
    // the blocks of one coefficient tile follow each other on their XCD: the next block of this residue is the tile's next coset
    if (b.coset + 1 < n_cosets) {
      const BlockId nx = decode_block((uint32_t)(L + g), log_g, n_tiles, n_cosets);
      CHECK(nx.tile == b.tile && nx.poly == b.poly && nx.coset == b.coset + 1, "block %llu: its XCD's next block is (%u, %u, %u)",
            (unsigned long long)L, nx.tile, nx.poly, nx.coset);
    }
    seen[((uint64_t)b.poly * n_tiles + b.tile) * n_cosets + b.coset]++;
  }
  for (uint8_t v : seen) CHECK(v == 1, "%u tiles, %u cosets, %u polys: a block seen %d times", n_tiles, n_cosets, n_polys, v);
  std::vector<uint8_t> blocks(n_cosets, 0);
  for (uint32_t c = 0; c < n_cosets; c++) {
    const uint32_t blk = coset_block(c, rb);
    CHECK(blk == rev(c, rb) && blk < n_cosets, "coset %u of 2^%d lands in block %u", c, rb, blk);
    if (blk < n_cosets) blocks[blk]++;
  }
  for (uint8_t v : blocks) CHECK(v == 1, "2^%d cosets: an output block written %d times", rb, v);
}

int main() {
  // every LDE the library accepts above rate 3 at its largest: log_n + rb = 24 (and the sizes below it at rb = 8)
  for (int rb = 4; rb <= 8; rb++)
    for (int log_n : {24 - rb, 11, 10, 6}) {
      if (log_n + rb > 24) continue;
      int l1, l2;
      split(log_n, l1, l2);
      if (l1 == 0) {   // single pass: one tile of one sub-transform per (polynomial, coset)
        check_pass2(Shape{l2, 0, 0, 256});
        check_decode(0, rb, 3);
        continue;
      }
      const int t1 = pick_log_t(l2, l1, true), t2 = pick_log_t(l1, l2 + rb, false);
      check_pass1(Shape{l2, t1, l1, (l2 + t1 >= 13) ? 512u : 256u});
      check_pass2(Shape{l1, t2, l2 + rb, (l1 + t2 >= 13) ? 512u : 256u});
      CHECK(l2 + rb <= 19 && l1 + l2 + rb <= 24, "pass 2 of log_n %d, rate %d: log_nt %d", log_n, rb, l2 + rb);
      check_decode((uint32_t)(l1 - t1), rb, log_n >= 16 ? 2 : 5);
    }
  // (log_nt = l2 + rb could reach 11 + 8 = 19 only at n = 2^22, an LDE of 2^30 words, which nothing accepts: the largest
  // accepted are log_nt = 16 at n = 2^16, rb = 8, above, and the rate-2 LDE of the largest transform, 2^22 points)
  check_pass2(Shape{11, 1, 13, 256});
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("NTT INDEX HIGH RATE OK (%ld elements)\n", checked);
  return 0;
}
