// The prover's numbers, each derived once: the pure size functions of the kernels, a circuit's dimensions (ProverShape) and
// the layout of the stand-alone FRI proof.  Host-only and free of HIP, so that a plain C++ program can check it
// (tests/native/working_set.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

namespace p25 {

// Words of a Merkle tree (kernels_hash.hip): levels 0 (leaf digests) .. log2(n) - cap_height (the cap), 4 words per node
inline size_t merkle_tree_words(size_t n_leaves, unsigned cap_height) {
  size_t total = 0;
  for (size_t m = n_leaves; m >= ((size_t)1 << cap_height); m >>= 1) {
    total += 4 * m;
    if (m == 1) break;
  }
  return total;
}

// Openings (kernels_fri.hip: k_eval_polys): one block per polynomial, lane t takes the coefficients k = t (mod S).
// S = 1024 lanes: the per-lane Horner chain (n / S dependent extension multiplies) is what a lone proof waits for.
constexpr uint32_t EVAL_LANES = 1024;
constexpr uint32_t EVAL_CHUNK_LOG = 16;  // polynomials longer than 2^16 are split into chunks, one block each
constexpr uint32_t EVAL_POW_WORDS = 2 * (EVAL_LANES + 2);  // one power table in the scratch
// scratch of launch_eval_jobs: the power tables, then the per-chunk partial sums of every polynomial
inline size_t eval_scratch_words(uint32_t n_points, size_t total_polys, uint32_t log_n) {
  const size_t chunks = log_n > EVAL_CHUNK_LOG ? (size_t)1 << (log_n - EVAL_CHUNK_LOG) : 1;
  return (size_t)n_points * EVAL_POW_WORDS + 2 * total_polys * chunks;
}

// A circuit's dimensions as the prover and the verifier use them.  Plain numbers: make_prover_shape (prover.h) fills one
// from a Circuit and its ProofLayout; DeviceCircuit keeps it.
struct ProverShape {
  int degree_bits, rate_bits;
  int quotient_bits;       // min(rate_bits, 3): the quotient has degree below 8n and is evaluated on 2^quotient_bits n points
  unsigned cap_height;
  size_t n, B, QB;         // rows; size of the LDE domain; of the quotient's coset (= B up to rate_bits 3)
  int W, NC, NP, nz, nq;   // wires, challenges, partial products per challenge, Z + partial-product polynomials, quotient chunks
  size_t capw, tw;         // words of a Merkle cap; of a tree over B leaves
  uint32_t oracle_width[4];   // constants|sigmas, wires, Zs|partial products, quotient chunks
  size_t total_polys;         // their sum
  std::vector<int> arity_bits;   // FRI reduction arities
  size_t proof_words;            // the flat proof's (ProofLayout::total)
  // words of the device transcript's, the challenge block's and the alpha-power table's buffers (prover_kernels.h, builder.h)
  size_t transcript_words, chal_words, alpha_pow_words;
};
// The derived numbers from the given ones.  width0: constants and sigmas; quotient_degree_factor: max_quotient_degree_factor.
inline ProverShape prover_shape(int degree_bits, int rate_bits, unsigned cap_height, int wires, int challenges,
                                int partial_products, int quotient_degree_factor, uint32_t width0, std::vector<int> arity_bits,
                                size_t proof_words, size_t transcript_words, size_t chal_words, size_t alpha_pow_words) {
  ProverShape s;
  s.degree_bits = degree_bits;
  s.rate_bits = rate_bits;
  s.cap_height = cap_height;
  s.n = (size_t)1 << degree_bits;
  s.B = s.n << rate_bits;
  s.quotient_bits = rate_bits < 3 ? rate_bits : 3;
  s.QB = s.n << s.quotient_bits;
  s.W = wires;
  s.NC = challenges;
  s.NP = partial_products;
  s.nz = challenges * (1 + partial_products);
  s.nq = challenges * quotient_degree_factor;
  s.capw = (size_t)4 << cap_height;
  s.tw = merkle_tree_words(s.B, cap_height);
  s.oracle_width[0] = width0;
  s.oracle_width[1] = (uint32_t)s.W;
  s.oracle_width[2] = (uint32_t)s.nz;
  s.oracle_width[3] = (uint32_t)s.nq;
  s.total_polys = (size_t)width0 + s.W + s.nz + s.nq;
  s.arity_bits = std::move(arity_bits);
  s.proof_words = proof_words;
  s.transcript_words = transcript_words;
  s.chal_words = chal_words;
  s.alpha_pow_words = alpha_pow_words;
  return s;
}

// FRI shape: shared by the whole-proof pipeline and the standalone p25_fri_prove entry point.
struct FriShape {
  int log_n, rate_bits;
  unsigned cap_height;
  std::vector<int> arity_bits;
  int pow_bits, num_queries;
};
struct FriOffsets {  // word offsets into the flat proof buffer
  size_t caps, final_poly, pow_witness, queries, query_stride;
};
// The stand-alone FRI proof (p25_fri_prove) of a shape whose layers fit (fri_prove_standalone checks): where the device
// writes CAP[n_layers] | final_poly | pow_witness | query openings, and the words of the host's output, which adds the
// betas (an extension element per layer) and the query indices.
struct FriStandaloneLayout {
  FriOffsets fo;
  size_t proof_words, out_words;
};
inline FriStandaloneLayout fri_standalone_layout(const FriShape& sh) {
  const size_t capw = (size_t)4 << sh.cap_height, nl = sh.arity_bits.size();
  int deg = sh.log_n, bits = sh.log_n + sh.rate_bits;
  size_t per_q = 0;
  for (int a : sh.arity_bits) {
    deg -= a;
    bits -= a;
    per_q += 2 * ((size_t)1 << a) + 4 * (size_t)(bits - (int)sh.cap_height);
  }
  FriStandaloneLayout l;
  l.fo.caps = 0;
  l.fo.final_poly = nl * capw;
  l.fo.pow_witness = l.fo.final_poly + 2 * ((size_t)1 << deg);
  l.fo.queries = l.fo.pow_witness + 1;
  l.fo.query_stride = per_q;
  l.proof_words = l.fo.queries + per_q * sh.num_queries;
  l.out_words = l.proof_words + 2 * nl + sh.num_queries;
  return l;
}

}  // namespace p25
