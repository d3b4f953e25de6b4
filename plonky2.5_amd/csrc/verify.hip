// Host side of the batch verifier: replaces `data.verify(proof)` (`src/p3/mod.rs:266` of the reference) for a batch of
// flat proofs.  The host only describes the batch (VerifyArgs: the proof layout and the circuit's shape) and enqueues
// the four launches of kernels_verify.hip on the circuit's main stream; nothing of a proving context is touched.
#include <string.h>
#include "prover.h"
#include "staging.h"
#include "verify_kernels.h"

namespace p25 {

// The batch description as far as the circuit alone decides it: shape, gate table, proof layout, the Merkle trees of
// a query round.  The caller adds the batch's pointers.  Refuses shapes the kernels do not hold.
VerifyArgs make_verify_args(const Circuit& c, const ProofLayout& L) {
  if (L.total >= ((size_t)1 << 32)) throw std::invalid_argument("proof too long for the verifier's 32-bit offsets");
  const ProverShape s = make_prover_shape(c, L);   // a DeviceCircuit's shape_; made here for a caller that has the circuit alone
  const std::vector<int>& ab = s.arity_bits;
  if (ab.size() > 8) throw std::invalid_argument("too many FRI layers");
  for (int b : ab)
    if (b < 1 || b > (int)VERIFY_MAX_ARITY_BITS) throw std::invalid_argument("FRI arity bits outside 1..5");
  if (c.cfg.num_query_rounds < 1 || c.cfg.num_query_rounds > 64) throw std::invalid_argument("1..64 query rounds are supported");
  if (s.NC != 2 || c.gates.size() > 16) throw std::invalid_argument("unsupported circuit configuration");
  VerifyArgs a;
  memset(&a, 0, sizeof(a));
  a.proof_words = (uint32_t)L.total;
  a.wires_cap = (uint32_t)L.wires_cap;
  a.zs_cap = (uint32_t)L.zs_cap;
  a.quotient_cap = (uint32_t)L.quotient_cap;
  a.constants = (uint32_t)L.constants;
  a.sigmas = (uint32_t)L.sigmas;
  a.wires = (uint32_t)L.wires;
  a.zs = (uint32_t)L.zs;
  a.zs_next = (uint32_t)L.zs_next;
  a.pps = (uint32_t)L.pps;
  a.quotient = (uint32_t)L.quotient;
  a.fri_caps = (uint32_t)L.fri_caps;
  a.queries = (uint32_t)L.queries;
  a.query_stride = (uint32_t)L.query_stride;
  a.final_poly = (uint32_t)L.final_poly;
  a.final_poly_len = L.final_poly_len;
  a.pow_witness = (uint32_t)L.pow_witness;
  a.public_inputs = (uint32_t)L.public_inputs;
  a.num_public_inputs = L.num_public_inputs;
  a.cap_words = (uint32_t)s.capw;
  a.degree_bits = (uint32_t)s.degree_bits;
  a.rate_bits = (uint32_t)s.rate_bits;
  a.pow_bits = (uint32_t)c.cfg.proof_of_work_bits;
  a.num_queries = (uint32_t)c.cfg.num_query_rounds;
  a.n_layers = (uint32_t)ab.size();
  a.num_selectors = (uint32_t)c.num_selectors;
  a.num_routed = (uint32_t)c.cfg.num_routed_wires;
  a.num_partial_products = (uint32_t)s.NP;
  a.quotient_degree_factor = (uint32_t)c.cfg.max_quotient_degree_factor;
  a.n_gates = (uint32_t)c.gates.size();
  for (uint32_t i = 0; i < a.n_gates; i++) {
    const int g = c.selector_index[i];
    a.gates[i] = GateEntry{(uint32_t)c.gates[i], (uint32_t)g, (uint32_t)c.groups[g].first, (uint32_t)c.groups[g].second};
  }
  // the Merkle trees of a query round, in the order the flat proof stores them
  const uint32_t lde_bits = a.degree_bits + a.rate_bits, cap_h = s.cap_height;
  const uint32_t caps[4] = {0, a.wires_cap, a.zs_cap, a.quotient_cap};
  uint32_t off = 0;
  for (int t = 0; t < 4; t++) {
    a.tree_off[t] = off;
    a.tree_width[t] = s.oracle_width[t];
    a.tree_depth[t] = lde_bits - cap_h;
    a.tree_shift[t] = 0;
    a.tree_cap[t] = caps[t];
    off += a.tree_width[t] + 4 * a.tree_depth[t];
  }
  uint32_t bits = lde_bits;
  for (uint32_t l = 0; l < a.n_layers; l++) {
    a.arity_bits[l] = (uint32_t)ab[l];
    bits -= a.arity_bits[l];
    a.tree_off[4 + l] = off;
    a.tree_width[4 + l] = 2u << a.arity_bits[l];
    a.tree_depth[4 + l] = bits - cap_h;
    a.tree_shift[4 + l] = lde_bits - bits;
    a.tree_cap[4 + l] = a.fri_caps + l * a.cap_words;
    off += a.tree_width[4 + l] + 4 * a.tree_depth[4 + l];
  }
  if (off != a.query_stride) throw std::logic_error("verifier: query round layout out of step with the proof layout");
  a.g_n = gl::root_of_unity(a.degree_bits);
  a.w_lde = gl::root_of_unity(lde_bits);
  return a;
}

void DeviceCircuit::verify_batch_dev(const u64* digest4, const u64* cs_cap, const u64* d_proofs, size_t n_proofs,
                                     size_t proof_stride, uint32_t* d_status) {
  if (proof_stride < layout_.total) throw std::invalid_argument("proof_stride smaller than the proof");
  if (n_proofs > ((size_t)1 << 24)) throw std::invalid_argument("more than 2^24 proofs in one batch");
  VerifyArgs a = make_verify_args(c_, layout_);
  const size_t capw = a.cap_words;
  if (digest4) {
    for (int i = 0; i < 4; i++)
      if (digest4[i] >= gl::P) throw std::invalid_argument("non-canonical digest word");
    for (size_t i = 0; i < capw; i++)
      if (cs_cap[i] >= gl::P) throw std::invalid_argument("non-canonical cap word");
  }
  // scratch: the caller's verifier data | challenge blocks | vanishing partials
  const size_t vd_words = 4 + capw, part_words = (size_t)(a.n_gates + 2) * 4;
  const size_t need = vd_words + n_proofs * (VCH_WORDS + part_words);
  if (verify_scratch_.words < need) {
    sync();   // an earlier batch may still be using the old allocation
    verify_scratch_.regrow(need);
  }
  a.proofs = d_proofs;
  a.stride = proof_stride;
  a.n_proofs = (uint32_t)n_proofs;
  a.k_is = k_is_.p;
  a.chal = verify_scratch_.p + vd_words;
  a.partial = a.chal + n_proofs * VCH_WORDS;
  a.status = d_status;
  if (digest4) {
    P25_HIP(hipMemcpyAsync(verify_scratch_.p, digest4, 32, hipMemcpyHostToDevice, stream_));
    P25_HIP(hipMemcpyAsync(verify_scratch_.p + 4, cs_cap, capw * 8, hipMemcpyHostToDevice, stream_));
    a.digest = verify_scratch_.p;
    a.cs_cap = verify_scratch_.p + 4;
  } else {
    a.digest = preamble_.p;
    a.cs_cap = cs_tree_.p + cs_tree_.words - capw;
  }
  stream_join(stream_);   // the proofs may still be on their way on the proving streams
  launch_verify_transcript(a, stream_);
  launch_verify_vanishing(a, stream_);
  launch_verify_fri(a, stream_);
  launch_verify_verdict(a, stream_);
  P25_HIP(hipGetLastError());
}

void DeviceCircuit::verify_batch(const u64* digest4, const u64* cs_cap, const u64* proofs, size_t n_proofs,
                                 size_t proof_stride, int32_t* statuses) {
  const size_t pw = layout_.total;
  if (proof_stride < pw) throw std::invalid_argument("proof_stride smaller than the proof");
  DevMem d_proofs(n_proofs * pw), d_status((n_proofs + 1) / 2 + 1);
  // the proof_stride - proof_words words behind a proof stay on the host: they are not read
  P25_HIP(hipMemcpy2DAsync(d_proofs.p, pw * 8, proofs, proof_stride * 8, pw * 8, n_proofs, hipMemcpyHostToDevice, stream_));
  verify_batch_dev(digest4, cs_cap, d_proofs.p, n_proofs, pw, (uint32_t*)d_status.p);
  statuses_to_host((const uint32_t*)d_status.p, n_proofs, statuses, stream_);
}

}  // namespace p25
