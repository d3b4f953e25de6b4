// Stand-alone check of the prover's sizing above rate 3 (plonky2.5_amd/csrc/prover_shape.h, working_set.h), beside
// working_set.cpp, which holds every buffer up to rate 3 to what it was.  The quotient has degree below 8n whatever the
// rate, so its values, the scratch of its inverse transform and its coefficients take QB = n << min(rate_bits, 3) words per
// challenge; everything that is committed (LDEs, trees, FRI layers) grows with B = n << rate_bits.  Against the counting
// test double of the HIP runtime (tests/native/fake_hip): a small context is constructed and requests exactly the sum.
#include <stdio.h>
#include <vector>
#include "working_set.h"

using namespace p25;

static int fails = 0;
#define CHECK(cond)                                   \
  do {                                                \
    if (!(cond) && fails++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr size_t TRANSCRIPT_WORDS = (12 + 8 + 8 + 1) + 1, CH_WORDS = 96, ALPHA_POWS = 192;
enum { WIRES_LDE = 3, WIRES_TREE = 4, ZS_LDE = 7, Q_VALS = 12, Q_TMP = 13, Q_COEFFS = 14, Q_LDE = 15, Q_TREE = 16, FRI0 = 24 };

static std::vector<size_t> table(const ProverShape& s) {
  std::vector<size_t> v;
  WorkingSet empty;
  empty.each_buffer(s, [&](DevMem&, size_t words) { v.push_back(words); });
  return v;
}

int main() {
  const int W = 135, NC = 2, NP = 9;
  size_t n_shapes = 0;
  for (int db : {2, 5, 11, 12, 16})
    for (int rb = 0; rb <= 8; rb++) {
      const int qf = 1 << (rb < 3 ? rb : 3);
      const std::vector<int> arity = db >= 11 ? std::vector<int>{4, 4} : std::vector<int>{};
      const ProverShape s = prover_shape(db, rb, 4 <= db + rb ? 4 : 0, W, NC, NP, qf, 85, arity, 7000, TRANSCRIPT_WORDS, CH_WORDS,
                                         2 * ALPHA_POWS);
      const size_t n = (size_t)1 << db, B = n << rb, QB = n << (rb < 3 ? rb : 3);
      CHECK(s.n == n && s.B == B && s.QB == QB && s.quotient_bits == (rb < 3 ? rb : 3) && s.nq == NC * qf);
      if (rb <= 3) CHECK(s.QB == s.B);
      const std::vector<size_t> t = table(s);
      CHECK(t.size() == FRI0 + 3 * arity.size() + 1 + 2);
      CHECK(t[WIRES_LDE] == W * B && t[ZS_LDE] == (size_t)NC * (1 + NP) * B && t[Q_LDE] == (size_t)NC * qf * B);
      CHECK(t[WIRES_TREE] == merkle_tree_words(B, s.cap_height) && t[Q_TREE] == t[WIRES_TREE]);
      CHECK(t[Q_VALS] == NC * QB && t[Q_TMP] == NC * QB && t[Q_COEFFS] == NC * QB);
      // the quotient's coefficients are its chunks: nq polynomials of n words, contiguous
      CHECK(t[Q_COEFFS] == (size_t)s.nq * n);
      // the FRI layers' values are on the LDE domain of the layer
      size_t m = n;
      for (size_t l = 0; l < arity.size(); l++) {
        CHECK(t[FRI0 + 3 * l] == 2 * m && t[FRI0 + 3 * l + 1] == 2 * (m << rb));
        CHECK(t[FRI0 + 3 * l + 2] == merkle_tree_words((m << rb) >> arity[l], s.cap_height));
        m >>= arity[l];
      }
      size_t sum = 0;
      for (size_t w : t) sum += w;
      CHECK(working_set_words(s) == sum);
      if (8 * sum <= ((size_t)64 << 20)) {   // constructed against the test double: it asks for exactly that
        g_fake_hip.bytes_requested = 0;
        {
          WorkingSet w(s);
          CHECK(g_fake_hip.bytes_requested == 8 * sum && w.q_vals.words == NC * QB && w.q_lde.words == (size_t)NC * qf * B);
        }
        CHECK(g_fake_hip.live() == 0 && g_fake_hip.bytes_live == 0 && g_fake_hip.bad_releases == 0);
      }
      n_shapes++;
    }
  // the 2^11-row shrink circuit at rate 8 against rate 3: committed buffers 32 times as large, the quotient's the same
  {
    const ProverShape a = prover_shape(11, 3, 4, W, NC, NP, 8, 85, {4, 4}, 15000, TRANSCRIPT_WORDS, CH_WORDS, 2 * ALPHA_POWS);
    const ProverShape b = prover_shape(11, 8, 4, W, NC, NP, 8, 85, {4, 4}, 7000, TRANSCRIPT_WORDS, CH_WORDS, 2 * ALPHA_POWS);
    const std::vector<size_t> ta = table(a), tb = table(b);
    CHECK(tb[WIRES_LDE] == 32 * ta[WIRES_LDE] && tb[Q_LDE] == 32 * ta[Q_LDE] && tb[Q_VALS] == ta[Q_VALS] && tb[Q_COEFFS] == ta[Q_COEFFS]);
    printf("2^11 rows: context bytes at rate 3 %zu, at rate 8 %zu\n", 8 * working_set_words(a), 8 * working_set_words(b));
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("WORKING SET HIGH RATE OK (%zu shapes)\n", n_shapes);
  return 0;
}
