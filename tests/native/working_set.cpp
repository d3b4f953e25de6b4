// Stand-alone check of the prover's sizing (plonky2.5_amd/csrc/prover_shape.h, working_set.h) against the counting test
// double of the HIP runtime (tests/native/fake_hip): over a grid of shapes, a context requests exactly the bytes the
// free-memory clamp counts for it, every buffer has the words the constructor of the commit before this table gave it
// (restated here, one line per buffer), a construction that fails at any creation gives everything back, and the
// stand-alone FRI proof's layout is the one stated here in numbers.  No GPU, no HIP.
//   working_set [max_bytes]    contexts above max_bytes are sized but not constructed (the sanitizer build: every block a
//                              context takes is a real malloc here); without it the whole grid is constructed
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "working_set.h"

using namespace p25;

static int fails = 0;
#define CHECK(cond)                                   \
  do {                                                \
    if (!(cond) && fails++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

static FakeHip& F = g_fake_hip;
static void settled() {
  CHECK(F.live() == 0 && F.bytes_live == 0);
  CHECK(F.bad_releases == 0);
  F.calls.clear();
  F.arm(0);
}

// what the library takes from its kernels' headers: sizeof(Transcript) / 8 + 1, CH_WORDS, 2 * ALPHA_POWS
constexpr size_t TRANSCRIPT_WORDS = (12 + 8 + 8 + 1) + 1, CH_WORDS = 96, ALPHA_POWS = 192;
constexpr int N_EVENTS = 2 + 12;

struct Dims {  // a shape as given by hand
  int degree_bits, rate_bits;
  unsigned cap_height;
  int wires, partial_products;
  uint32_t width0;
  std::vector<int> arity;
  size_t proof_words;
};
static ProverShape shape_of(const Dims& d) {
  return prover_shape(d.degree_bits, d.rate_bits, d.cap_height, d.wires, 2, d.partial_products, 8, d.width0, d.arity,
                      d.proof_words, TRANSCRIPT_WORDS, CH_WORDS, 2 * ALPHA_POWS);
}
// every FRI layer, and the final polynomial, at least as large as the Merkle cap
static bool fits(const Dims& d) {
  int deg = d.degree_bits, bits = d.degree_bits + d.rate_bits;
  for (int a : d.arity) {
    deg -= a;
    bits -= a;
  }
  return deg >= 0 && bits >= (int)d.cap_height;
}

// The sizes as the constructor of a context and FriWork::alloc stated them before there was a table: their expressions as
// they stood, in allocation order.  c / L stand for the circuit and its proof layout.
static std::vector<size_t> sizes_before(const Dims& d) {
  struct {
    int degree_bits;
    struct { int rate_bits; unsigned cap_height; int num_wires, num_challenges, max_quotient_degree_factor; } cfg;
    int num_partial_products;
    std::vector<int> fri_reduction_arity_bits;
    size_t degree() const { return (size_t)1 << degree_bits; }
  } c{d.degree_bits, {d.rate_bits, d.cap_height, d.wires, 2, 8}, d.partial_products, d.arity};
  struct { uint32_t oracle_width[4]; size_t total; } L;
  L.oracle_width[0] = d.width0;
  L.oracle_width[1] = (uint32_t)c.cfg.num_wires;
  L.oracle_width[2] = (uint32_t)(c.cfg.num_challenges * (1 + c.num_partial_products));
  L.oracle_width[3] = (uint32_t)(c.cfg.num_challenges * c.cfg.max_quotient_degree_factor);
  L.total = d.proof_words;
  std::vector<size_t> v;
  const size_t n = c.degree(), B = c.degree() << c.cfg.rate_bits;
  const int W = c.cfg.num_wires, NC = c.cfg.num_challenges, NP = c.num_partial_products;
  const int nz = NC * (1 + NP), nq = NC * c.cfg.max_quotient_degree_factor;
  const size_t tw = merkle_tree_words(B, c.cfg.cap_height);
  v.push_back((size_t)W * n);                                          // wires_vals
  v.push_back((size_t)W * n);                                          // wires_coeffs
  v.push_back((size_t)W * n);                                          // tmp
  v.push_back((size_t)W * B);                                          // wires_lde
  v.push_back(tw);                                                     // wires_tree
  v.push_back((size_t)nz * n);                                         // zs_vals
  v.push_back((size_t)nz * n);                                         // zs_coeffs
  v.push_back((size_t)nz * B);                                         // zs_lde
  v.push_back(tw);                                                     // zs_tree
  v.push_back((size_t)NC * (NP + 1) * n);                              // zpp_chunk
  v.push_back((size_t)NC * n);                                         // zpp_tot
  v.push_back((size_t)NC * ((n + 255) / 256) + 16);                    // zpp_btot
  v.push_back((size_t)NC * B);                                         // q_vals
  v.push_back((size_t)NC * B);                                         // q_tmp
  v.push_back((size_t)NC * B);                                         // q_coeffs
  v.push_back((size_t)nq * B);                                         // q_lde
  v.push_back(tw);                                                     // q_tree
  v.push_back(8);                                                      // preamble
  v.push_back(TRANSCRIPT_WORDS);                                       // transcript
  v.push_back(CH_WORDS);                                               // chal
  v.push_back(2 * ALPHA_POWS);                                         // alpha_pows
  v.push_back(eval_scratch_words(2, (size_t)L.oracle_width[0] + W + nz + nq + NC, (uint32_t)c.degree_bits));   // eval_pows
  v.push_back(4 * n);                                                  // fri_comp
  const size_t total_polys = L.oracle_width[0] + L.oracle_width[1] + L.oracle_width[2] + L.oracle_width[3];
  v.push_back(2 * (total_polys + 1) + 8 * (n + 1) + 4 * ((n + 255) / 256) + 64);   // fri_scan
  {  // fri.alloc(c.degree_bits, c.cfg.rate_bits, c.cfg.cap_height, c.fri_reduction_arity_bits)
    const int log_n = c.degree_bits, rate_bits = c.cfg.rate_bits;
    const unsigned cap_height = c.cfg.cap_height;
    const std::vector<int>& arity_bits = c.fri_reduction_arity_bits;
    size_t m = (size_t)1 << log_n;
    const size_t nl = arity_bits.size();
    for (size_t l = 0; l <= nl; l++) {
      v.push_back(2 * m);                                              // coeffs[l]
      if (l < nl) {
        size_t nvals = m << rate_bits;
        v.push_back(2 * nvals);                                        // vals[l]
        v.push_back(merkle_tree_words(nvals >> arity_bits[l], cap_height));   // tree[l]
        m >>= arity_bits[l];
      }
    }
  }
  v.push_back(L.total);                                                // proof
  v.push_back(1);                                                      // status
  return v;
}
// the buffers of a constructed context in the same order, by name
static std::vector<const DevMem*> buffers_of(const WorkingSet& w, size_t n_layers) {
  std::vector<const DevMem*> v = {&w.wires_vals, &w.wires_coeffs, &w.tmp, &w.wires_lde, &w.wires_tree, &w.zs_vals, &w.zs_coeffs,
                                  &w.zs_lde, &w.zs_tree, &w.zpp_chunk, &w.zpp_tot, &w.zpp_btot, &w.q_vals, &w.q_tmp, &w.q_coeffs,
                                  &w.q_lde, &w.q_tree, &w.preamble, &w.transcript, &w.chal, &w.alpha_pows, &w.eval_pows,
                                  &w.fri_comp, &w.fri_scan};
  for (size_t l = 0; l <= n_layers; l++) {
    v.push_back(&w.fri.coeffs[l]);
    if (l < n_layers) {
      v.push_back(&w.fri.vals[l]);
      v.push_back(&w.fri.tree[l]);
    }
  }
  v.push_back(&w.proof);
  v.push_back(&w.status);
  return v;
}
// the memory formula the clamp used before (DeviceCircuit::ctx_bytes of the commit before), for the report
static size_t bytes_before(const Dims& d) {
  const size_t n = (size_t)1 << d.degree_bits, B = (size_t)1 << (d.degree_bits + d.rate_bits);
  const size_t W = d.wires, NC = 2, NP = d.partial_products;
  const size_t nz = NC * (1 + NP), nq = NC * 8;
  const size_t tw = merkle_tree_words(B, d.cap_height);
  return 8 * (3 * W * n + W * B + 2 * nz * n + nz * B + 3 * NC * B + nq * B + 3 * tw + 16 * n + 6 * B);
}

static size_t n_sized = 0, n_built = 0;
static void check_shape(const Dims& d, size_t max_bytes) {
  const ProverShape s = shape_of(d);
  const std::vector<size_t> want = sizes_before(d);
  size_t n_buffers = 0, sum = 0;
  const size_t bytes = 8 * working_set_words(s, &n_buffers);
  for (size_t w : want) sum += w;
  CHECK(n_buffers == want.size() && bytes == 8 * sum);
  {  // the table itself, without allocating
    WorkingSet empty;
    size_t i = 0;
    empty.each_buffer(s, [&](DevMem&, size_t words) {
      CHECK(i < want.size() && words == want[i] && words > 0);
      i++;
    });
  }
  n_sized++;
  if (bytes > max_bytes) return;
  n_built++;
  {
    WorkingSet w(s);
    CHECK(F.bytes_requested == bytes && F.bytes_live == bytes);
    CHECK(F.mem.size() == n_buffers && F.events.size() == (size_t)N_EVENTS && F.creations == n_buffers + N_EVENTS);
    // the events come first and last, the buffers one hipMalloc each between them
    CHECK(F.calls == "EE" + std::string(n_buffers, 'M') + std::string(12, 'E'));
    const std::vector<const DevMem*> got = buffers_of(w, d.arity.size());
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++) CHECK(got[i]->p && got[i]->words == want[i]);
  }
  F.bytes_requested = 0;
  settled();
  for (size_t nth = 1; nth <= n_buffers + N_EVENTS; nth++) {
    F.arm(nth);
    bool threw = false;
    try {
      WorkingSet w(s);
    } catch (const HipError&) {
      threw = true;
    }
    CHECK(threw && F.creations == nth);
    settled();
  }
  F.arm(n_buffers + N_EVENTS + 1);   // there is no such creation
  {
    WorkingSet w(s);
    CHECK(w.status.p);
  }
  F.bytes_requested = 0;
  settled();
}

static void test_grid(size_t max_bytes) {
  const std::vector<std::vector<int>> arities = {{}, {1}, {4}, {4, 4, 4}, {4, 4, 4, 4}};
  for (int db : {2, 7, 12, 16, 19})
    for (int rb : {1, 2, 3})
      for (unsigned cap : {0u, 4u})
        for (int wires : {80, 135})
          for (int np : {1, 2, 9})
            for (uint32_t w0 : {4u, 85u})
              for (const auto& ar : arities) {
                const Dims d{db, rb, cap, wires, np, w0, ar, 1000 + 97 * (size_t)db + 4 * ar.size()};
                if (fits(d)) check_shape(d, max_bytes);
              }
  CHECK(n_sized > 1000 && n_built > 0);
}

static void test_merkle_and_eval_words() {
  // a tree over 2^k leaves with a cap of 2^h nodes: levels 2^k .. 2^h, 4 words a node
  for (unsigned k = 0; k <= 22; k++)
    for (unsigned h = 0; h <= k && h <= 5; h++) CHECK(merkle_tree_words((size_t)1 << k, h) == 4 * (((size_t)2 << k) - ((size_t)1 << h)));
  CHECK(merkle_tree_words(8, 4) == 0);   // a cap above the leaves has no tree
  CHECK(eval_scratch_words(2, 258, 16) == 2 * 2052 + 2 * 258);
  CHECK(eval_scratch_words(2, 258, 19) == 2 * 2052 + 2 * 258 * 8);
  CHECK(eval_scratch_words(1, 3, 2) == 2052 + 6);
}

// The stand-alone FRI proof at rate_bits 3, cap_height 2, 28 queries: the words of p25_fri_prove's output and the offsets
// its device proof is written at, as the commit before computed them (fri_prove_words, fri_prove_standalone)
static void test_fri_layout() {
  struct Case {
    int log_n;
    std::vector<int> arity;
    size_t words;
    FriOffsets fo;
  };
  const Case cases[] = {
      {4, {}, 61, {0, 0, 32, 33, 0}},
      {4, {1}, 623, {0, 16, 32, 33, 20}},
      {4, {4}, 1057, {0, 16, 18, 19, 36}},
      {8, {}, 541, {0, 0, 512, 513, 0}},
      {8, {1}, 1311, {0, 16, 272, 273, 36}},
      {8, {4}, 1535, {0, 16, 48, 49, 52}},
      {16, {}, 131101, {0, 0, 131072, 131073, 0}},
      {16, {1}, 67487, {0, 16, 65552, 65553, 68}},
      {16, {4}, 10591, {0, 16, 8208, 8209, 84}},
      {16, {4, 4, 4}, 5827, {0, 48, 80, 81, 204}},
      {16, {4, 4, 4, 4}, 6823, {0, 64, 66, 67, 240}},
  };
  for (const Case& k : cases) {
    const FriShape sh{k.log_n, 3, 2, k.arity, 16, 28};
    const FriStandaloneLayout l = fri_standalone_layout(sh);
    CHECK(l.out_words == k.words);
    CHECK(l.fo.caps == k.fo.caps && l.fo.final_poly == k.fo.final_poly && l.fo.pow_witness == k.fo.pow_witness &&
          l.fo.queries == k.fo.queries && l.fo.query_stride == k.fo.query_stride);
    CHECK(l.proof_words == k.fo.queries + k.fo.query_stride * 28);
  }
}

// the two circuits DESIGN.md section 2 speaks of: the verifier circuit of the 64-row Fibonacci STARK, and BASELINE config 5's
static void report() {
  const Dims fib64{16, 3, 4, 135, 9, 85, {4, 4, 4}, 19861}, config5{19, 3, 4, 135, 9, 85, {4, 4, 4, 4}, 23381};
  const Dims* both[2] = {&fib64, &config5};
  const char* names[2] = {"fib-64", "config-5"};
  for (int i = 0; i < 2; i++)
    printf("%s: context bytes by the formula before %zu, exact %zu\n", names[i], bytes_before(*both[i]),
           8 * working_set_words(shape_of(*both[i])));
}

int main(int argc, char** argv) {
  const size_t max_bytes = argc > 1 ? (size_t)strtoull(argv[1], nullptr, 10) : (size_t)-1;
  test_merkle_and_eval_words();
  test_fri_layout();
  test_grid(max_bytes);
  report();
  printf("%zu shapes sized, %zu of them constructed\n", n_sized, n_built);
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("WORKING_SET OK\n");
  return 0;
}
