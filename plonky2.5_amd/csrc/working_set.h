// The device memory of a proof in flight, stated once: each_buffer is the table of a context's buffers, every one with its
// words as a function of the ProverShape, in allocation order.  The constructor allocates from it and working_set_words
// sums it, so the free-memory clamp of prove_batch_dev divides by what a context really takes.  Needs dev_res.h's part of
// the HIP runtime only: tests/native/working_set.cpp checks it against the counting test double.
#pragma once
#include <stdexcept>
#include "dev_res.h"
#include "prover_shape.h"

namespace p25 {

// FRI working set: shared by the whole-proof pipeline and the standalone p25_fri_prove entry point.
struct FriWork {
  DevMem coeffs[9], vals[9], tree[9];
  // f(buffer, words) per layer: the polynomial's coefficients (components a | b), and for a layer that is folded its
  // values on the LDE domain and the Merkle tree over their leaves
  template <class F>
  void each_buffer(int log_n, int rate_bits, unsigned cap_height, const std::vector<int>& arity_bits, F&& f) {
    size_t m = (size_t)1 << log_n;
    const size_t nl = arity_bits.size();
    if (nl > 8) throw std::invalid_argument("too many FRI layers");
    for (size_t l = 0; l <= nl; l++) {
      f(coeffs[l], 2 * m);
      if (l < nl) {
        const size_t nvals = m << rate_bits;
        f(vals[l], 2 * nvals);
        f(tree[l], merkle_tree_words(nvals >> arity_bits[l], cap_height));
        m >>= arity_bits[l];
      }
    }
  }
  void alloc(int log_n, int rate_bits, unsigned cap_height, const std::vector<int>& arity_bits) {
    each_buffer(log_n, rate_bits, cap_height, arity_bits, [](DevMem& m, size_t words) { m = DevMem(words); });
  }
};

// Everything a context owns: a constructor that throws half way gives back what it had made.
struct WorkingSet {
  // done[b]: recorded after the context's latest read of witness-value buffer b (DeviceCircuit::vals_[b])
  DevEvent done[2];
  DevMem wires_vals, wires_coeffs, tmp, wires_lde, wires_tree;
  DevMem zs_vals, zs_coeffs, zs_lde, zs_tree, zpp_chunk, zpp_tot, zpp_btot;
  DevMem q_vals, q_tmp, q_coeffs, q_lde, q_tree;
  DevMem preamble;  // circuit_digest[4] | public_inputs_hash[4] of the proof in flight: what the transcript absorbs first
  DevMem transcript, chal, alpha_pows, eval_pows;
  DevMem fri_comp, fri_scan;
  FriWork fri;
  DevMem proof, status;
  DevEvent ev[12];  // PhaseTimes marks

  WorkingSet() {}
  explicit WorkingSet(const ProverShape& s) {
    for (auto& e : done) e.create(hipEventDisableTiming);
    each_buffer(s, [](DevMem& m, size_t words) { m = DevMem(words); });
    for (auto& e : ev) e.create();
  }
  template <class F>
  void each_buffer(const ProverShape& s, F&& f) {
    const size_t n = s.n, B = s.B, QB = s.QB, W = s.W, NC = s.NC, NP = s.NP, nz = s.nz, nq = s.nq, blocks = (n + 255) / 256;
    f(wires_vals, W * n);
    f(wires_coeffs, W * n);
    f(tmp, W * n);
    f(wires_lde, W * B);
    f(wires_tree, s.tw);
    f(zs_vals, nz * n);
    f(zs_coeffs, nz * n);
    f(zs_lde, nz * B);
    f(zs_tree, s.tw);
    f(zpp_chunk, NC * (NP + 1) * n);
    f(zpp_tot, NC * n);
    f(zpp_btot, NC * blocks + 16);
    f(q_vals, NC * QB);
    f(q_tmp, NC * QB);
    f(q_coeffs, NC * QB);
    f(q_lde, nq * B);
    f(q_tree, s.tw);
    f(preamble, 8);
    f(transcript, s.transcript_words);
    f(chal, s.chal_words);
    f(alpha_pows, s.alpha_pow_words);
    // the power tables of zeta and g zeta, followed by the per-chunk partial sums of the openings (launch_eval_jobs)
    f(eval_pows, eval_scratch_words(2, s.total_polys + NC, (uint32_t)s.degree_bits));
    f(fri_comp, 4 * n);
    f(fri_scan, 2 * (s.total_polys + 1) + 8 * (n + 1) + 4 * blocks + 64);
    fri.each_buffer(s.degree_bits, s.rate_bits, s.cap_height, s.arity_bits, f);
    f(proof, s.proof_words);
    f(status, 1);
  }
};

// words of one context's buffers, and how many buffers there are: the table read without allocating
inline size_t working_set_words(const ProverShape& s, size_t* n_buffers = nullptr) {
  WorkingSet empty;
  size_t total = 0, count = 0;
  empty.each_buffer(s, [&](DevMem&, size_t words) {
    total += words;
    count++;
  });
  if (n_buffers) *n_buffers = count;
  return total;
}

}  // namespace p25
