// Internal: the batch verifier's kernel arguments and launchers (kernels_verify.hip).  One VerifyArgs describes a whole
// batch: every stage is launched once over all its proofs.
#pragma once
#include "prover_kernels.h"

namespace p25 {

// per-proof scratch block (u64 words): the CH_* challenge block of prover_kernels.h, then the public-inputs hash
enum { VCH_PI_HASH = CH_WORDS, VCH_WORDS = CH_WORDS + 4 };
constexpr uint32_t VERIFY_MAX_TREES = 12;     // the 4 initial oracles + up to 8 FRI layers
constexpr uint32_t VERIFY_MAX_ARITY_BITS = 5;

// While a batch is being checked, a proof's status word holds the KEY of the earliest failed check found so far
// (atomicMin: lanes that check in parallel reduce to the first failure of the sequential verifier, not to the last
// writer); the verdict kernel turns it into the P25_REJECT_* code.
enum : uint32_t {
  VKEY_MALFORMED = 0, VKEY_VANISHING = 1, VKEY_POW = 2,
  VKEY_QUERY = 3,          // + query * VKEY_QUERY_STEPS + step: steps 0..3 the initial Merkle paths, then per FRI layer
  VKEY_QUERY_STEPS = 32,   //   l the evaluation check (4 + 2 l) and the layer's Merkle path (5 + 2 l), then the final
  VKEY_NONE = 0xFFFFFFFFu  //   polynomial (4 + 2 n_layers)
};
enum : uint32_t {  // include/p25.h: P25_REJECT_*
  V_REJECT_VANISHING = 20, V_REJECT_POW = 21, V_REJECT_MALFORMED = 22, V_REJECT_INITIAL_MERKLE = 23, V_REJECT_FRI_EVAL = 24,
  V_REJECT_FRI_MERKLE = 25, V_REJECT_FINAL_POLY = 26
};

struct VerifyArgs {
  const u64* proofs;   // proof p = proof_words words at proofs + p * stride
  size_t stride;
  uint32_t n_proofs;
  const u64* digest;   // [4] circuit digest
  const u64* cs_cap;   // [cap_words] constants/sigmas cap
  const u64* k_is;     // [num_routed]
  u64* chal;           // scratch [n_proofs][VCH_WORDS]
  u64* partial;        // scratch [n_proofs][n_gates + 2][4]: each vanishing task's share of the two alpha folds
  uint32_t* status;    // [n_proofs]
  // flat proof layout (include/p25.h), word offsets
  uint32_t proof_words, wires_cap, zs_cap, quotient_cap, constants, sigmas, wires, zs, zs_next, pps, quotient, fri_caps,
      queries, query_stride, final_poly, final_poly_len, pow_witness, public_inputs, num_public_inputs;
  uint32_t cap_words, degree_bits, rate_bits, pow_bits, num_queries, n_layers;
  uint32_t num_selectors, num_routed, num_partial_products, quotient_degree_factor, n_gates;
  GateEntry gates[16];
  uint32_t arity_bits[8];
  // Merkle trees opened per query: where the leaf starts inside a query round, its width, the number of siblings behind
  // it, the shift that takes the query index to the leaf index, and where the cap is in the proof (tree 0: cs_cap)
  uint32_t tree_off[VERIFY_MAX_TREES], tree_width[VERIFY_MAX_TREES], tree_depth[VERIFY_MAX_TREES],
      tree_shift[VERIFY_MAX_TREES], tree_cap[VERIFY_MAX_TREES];
  u64 g_n;     // generator of the size-n subgroup: zeta_next = g_n * zeta
  u64 w_lde;   // primitive root of the LDE domain
};

// the circuit's part of a batch description (verify.hip); the caller fills in the pointers and n_proofs
struct Circuit;
struct ProofLayout;
VerifyArgs make_verify_args(const Circuit& c, const ProofLayout& layout);

// 1. Fiat-Shamir replay + canonical-word scan: chal block and public-inputs hash per proof, status = VKEY_NONE / VKEY_MALFORMED
void launch_verify_transcript(const VerifyArgs& a, hipStream_t st);
// 2. vanishing(zeta): every (gate type | permutation argument of one challenge) x proof is one lane -> partial
void launch_verify_vanishing(const VerifyArgs& a, hipStream_t st);
// 3. FRI queries: one lane per (proof, query, tree) Merkle path and one per (proof, query) for the arithmetic
void launch_verify_fri(const VerifyArgs& a, hipStream_t st);
// 4. per proof: sum of the partials against Z_H(zeta) t(zeta), the PoW response, key -> P25_REJECT_* code
void launch_verify_verdict(const VerifyArgs& a, hipStream_t st);

}  // namespace p25
