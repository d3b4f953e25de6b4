// Stand-alone check of ntt_index.h (no GPU, no HIP): the cursors that k_ntt_tile advances from element to element give the
// addresses of the closed forms, a block's load map and store map are bijections between its tile and its LDS slots, and the
// blocks of a launch cover a polynomial exactly once.
//
// The closed forms, from the header comment of kernels_ntt.hip -- element (t, i): sub-transform t, element i of it:
//   kind 0 ("t-contiguous"): addr = t + imap(i) * NT
//   kind 1 ("i-contiguous"): addr = tmap(t) * R + imap(i)
// with imap / tmap the identity or a bit reversal.  Element e of a block (e = tid + k * nth) is (t, i) = (e mod T, e / T)
// in kind 0 and the word e of the block's T rows in kind 1; it lives in LDS slot i * TP + t.  After the DIF network LDS
// position q of a sub-transform holds frequency j = rev(q).
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
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

static uint32_t rev(uint32_t x, int bits) {
  uint32_t r = 0;
  for (int b = 0; b < bits; b++)
    if (x >> b & 1) r |= 1u << (bits - 1 - b);
  return r;
}

struct Shape {
  int log_r, log_t, log_nt;
  uint32_t nth;
};
struct Where {
  uint32_t addr, slot, t, i_or_j;
};

// today's in_slot, restated
static Where load_closed(int form, const Shape& s, uint32_t tg0, uint32_t e) {
  const uint32_t T = 1u << s.log_t, R = 1u << s.log_r, NT = 1u << s.log_nt, TP = T > 1 ? T + 1 : 1;
  uint32_t t, i, addr;
  if (form == IN_T) {
    t = e & (T - 1), i = e >> s.log_t;
    addr = (tg0 + t) + i * NT;
  } else {
    const uint32_t off = e & (R - 1);
    t = e >> s.log_r;
    i = form == IN_I_BR ? rev(off, s.log_r) : off;
    const uint32_t trow = form == IN_I_BR ? rev(tg0 + t, s.log_nt) : tg0 + t;
    addr = trow * R + off;
  }
  return Where{addr, i * TP + t, t, i};
}
// today's out_slot, restated
static Where store_closed(int form, const Shape& s, uint32_t tg0, uint32_t e) {
  const uint32_t T = 1u << s.log_t, R = 1u << s.log_r, NT = 1u << s.log_nt, TP = T > 1 ? T + 1 : 1;
  uint32_t t, q, j, addr;
  if (form == OUT_T || form == OUT_T_BR) {
    t = e & (T - 1), q = e >> s.log_t;
    j = rev(q, s.log_r);
    addr = (tg0 + t) + (form == OUT_T_BR ? q : j) * NT;
  } else {
    const uint32_t off = e & (R - 1);
    t = e >> s.log_r;
    q = form == OUT_I_BR ? off : rev(off, s.log_r);
    j = rev(q, s.log_r);
    addr = (tg0 + t) * R + off;
  }
  return Where{addr, q * TP + t, t, j};
}

// One launch: every tile's block, every lane, every element.  `load`: the cursor is a LoadCursor<FORM>, else a StoreCursor.
template <bool LOAD, int FORM>
static void check_launch(const Shape& s) {
  const uint32_t T = 1u << s.log_t, R = 1u << s.log_r, NT = 1u << s.log_nt, TP = T > 1 ? T + 1 : 1, TR = T * R;
  std::vector<uint8_t> poly((size_t)NT * R, 0);
  std::vector<uint8_t> slots, elems;
  for (uint32_t tile = 0; tile < NT / T; tile++) {
    const Tile tl{s.log_r, s.log_t, s.log_nt, tile * T};
    slots.assign((size_t)R * TP, 0);
    elems.assign(TR, 0);
    for (uint32_t tid = 0; tid < s.nth; tid++) {
      typename std::conditional<LOAD, LoadCursor<FORM>, StoreCursor<FORM>>::type c;
      c.init(tl, tid, s.nth);
      for (uint32_t e = tid; e < TR; e += s.nth, c.next()) {
        checked++;
        Where w;
        uint32_t second;
        if constexpr (LOAD) {
          w = load_closed(FORM, s, tl.tg0, e);
          second = c.idx();
        } else {
          w = store_closed(FORM, s, tl.tg0, e);
          second = c.j();
          CHECK(c.tw() == tl.tg0 + w.t, "form %d r %d t %d nt %d nth %u tile %u e %u: tw %u", FORM, s.log_r, s.log_t, s.log_nt,
                s.nth, tile, e, c.tw());
          CHECK((uint64_t)c.tw() * c.j() < ((uint64_t)1 << 22) && c.tw() < (1u << 24) && c.j() < (1u << 24),
                "twiddle index out of the 24-bit product's range: %u * %u", c.tw(), c.j());
        }
        CHECK(c.goff() == w.addr && c.slot() == w.slot && second == w.i_or_j,
              "%s form %d r %d t %d nt %d nth %u tile %u e %u: cursor (%u, %u, %u) closed form (%u, %u, %u)", LOAD ? "load" : "store",
              FORM, s.log_r, s.log_t, s.log_nt, s.nth, tile, e, c.goff(), c.slot(), second, w.addr, w.slot, w.i_or_j);
        // the element of the tile this is: each once, each in a slot of its own, each at a word of its own
        const uint32_t el = w.t * R + w.i_or_j;
        if (w.t >= T || w.i_or_j >= R || w.slot >= R * TP || w.addr >= NT * R) {
          CHECK(false, "out of range: form %d r %d t %d nt %d e %u", FORM, s.log_r, s.log_t, s.log_nt, e);
          continue;
        }
        CHECK(!elems[el]++, "element (%u, %u) twice", w.t, w.i_or_j);
        CHECK(!slots[w.slot]++, "slot %u twice", w.slot);
        CHECK(!poly[w.addr]++, "word %u of the polynomial twice (tile %u)", w.addr, tile);
        // and the word is where the kind's definition puts that element
        const uint32_t tg = tl.tg0 + w.t, x = w.i_or_j;
        uint32_t def;
        if (LOAD) def = FORM == IN_T ? tg + x * NT : FORM == IN_I ? tg * R + x : rev(tg, s.log_nt) * R + rev(x, s.log_r);
        else def = FORM == OUT_T ? tg + x * NT : FORM == OUT_T_BR ? tg + rev(x, s.log_r) * NT : FORM == OUT_I ? tg * R + x
                                                                                                  : tg * R + rev(x, s.log_r);
        CHECK(def == w.addr, "form %d: element (%u, %u) belongs at %u, not %u", FORM, tg, x, def, w.addr);
      }
    }
    size_t n_el = 0, n_sl = 0;
    for (uint8_t v : elems) n_el += v == 1;
    for (uint8_t v : slots) n_sl += v == 1;
    CHECK(n_el == TR && n_sl == TR, "form %d r %d t %d nt %d nth %u tile %u: %zu elements, %zu slots of %u", FORM, s.log_r,
          s.log_t, s.log_nt, s.nth, tile, n_el, n_sl, TR);
  }
  size_t n = 0;
  for (uint8_t v : poly) n += v == 1;
  CHECK(n == (size_t)NT * R, "form %d r %d t %d nt %d nth %u: %zu of %zu words covered once", FORM, s.log_r, s.log_t, s.log_nt,
        s.nth, n, (size_t)NT * R);
}

static void check_shape(const Shape& s) {
  check_launch<true, IN_T>(s);
  check_launch<true, IN_I>(s);
  check_launch<true, IN_I_BR>(s);
  check_launch<false, OUT_T>(s);
  check_launch<false, OUT_T_BR>(s);
  check_launch<false, OUT_I>(s);
  check_launch<false, OUT_I_BR>(s);
}

int main() {
  for (uint32_t nth : {256u, 512u})
    for (int log_r = 1; log_r <= 11; log_r++)
      for (int log_t = 0; log_t <= 4; log_t++)
        for (int log_nt : {log_t, log_t + 1, log_t + 4})   // one tile, two tiles, sixteen tiles
          check_shape(Shape{log_r, log_t, log_nt, nth});
  // shapes the library launches: 2^16 points (both passes, and pass 2 over the 8 cosets of an LDE), 2^19 points, and the
  // largest transform it accepts, 2^22 points
  for (const Shape& s : {Shape{8, 4, 8, 256}, Shape{8, 4, 11, 256}, Shape{9, 4, 10, 512}, Shape{10, 3, 9, 512}, Shape{11, 1, 11, 256}})
    check_shape(s);
  // the block decode: every (tile, polynomial, coset) once
  for (uint32_t log_tiles = 0; log_tiles <= 7; log_tiles++)
    for (uint32_t n_cosets : {1u, 2u, 8u})
      for (uint32_t n_polys : {1u, 3u}) {
        const uint32_t n_tiles = 1u << log_tiles;
        uint32_t log_g = 0;
        while (log_g < 3 && (2u << log_g) <= n_tiles) log_g++;
        std::vector<int> seen((size_t)n_tiles * n_cosets * n_polys, 0);
        for (uint32_t L = 0; L < seen.size(); L++) {
          const BlockId b = decode_block(L, log_g, n_tiles, n_cosets);
          if (b.tile >= n_tiles || b.poly >= n_polys || b.coset >= n_cosets) {
            CHECK(false, "block %u of %u tiles, %u cosets, %u polys: (%u, %u, %u)", L, n_tiles, n_cosets, n_polys, b.tile, b.poly, b.coset);
            continue;
          }
          CHECK((b.tile & ((1u << log_g) - 1)) == (L & ((1u << log_g) - 1)), "block %u: tile %u on another XCD", L, b.tile);
          seen[((size_t)b.poly * n_tiles + b.tile) * n_cosets + b.coset]++;
        }
        for (int v : seen) CHECK(v == 1, "%u tiles, %u cosets, %u polys: a block seen %d times", n_tiles, n_cosets, n_polys, v);
      }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("NTT INDEX OK (%ld elements)\n", checked);
  return 0;
}
