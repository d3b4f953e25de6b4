// Host side of the plonky3 batch verifier: describes the batch (P3VerifyArgs: the proof's layout and the shape's constants)
// and enqueues the five launches of kernels_p3_verify.hip, a chunk of proofs at a time.  It shares the handle's AIR program
// and event chain with the prover (p3_prover_dev.hip) and none of its scratch.
#include <algorithm>
#include "p3_prover_impl.h"
#include "staging.h"
#include "p3_verify_lanes.h"

namespace p25 {

size_t P3ProverDev::verify_scratch_words_per_proof() const {
  return p3v_scratch_words(shape_.k, shape_.num_queries, shape_.AW ? shape_.NC : 0);   // the challenge block grows by 2 NC
}
size_t P3ProverDev::verify_chunk(size_t n_proofs) const {
  const size_t c = std::min(budget_bytes_, P3_VERIFY_SCRATCH_BYTES) / (verify_scratch_words_per_proof() * 8);
  return std::min(std::max<size_t>(1, c), n_proofs);
}
void P3ProverDev::scratch_bytes(size_t* proving, size_t* verifying) const {
  if (proving) *proving = impl_ ? (impl_->scratch.words + impl_->prep.words + impl_->check_tab.words) * 8 : 0;   // the preprocessed tables and the checker's count here
  if (verifying) *verifying = impl_ ? impl_->vscratch.words * 8 : 0;
}

// The batch description as far as the handle decides it: the proof's layout, the shape's constants and the AIR program
// (host pointers; verify_dev puts the device copies in their place).  The caller adds the batch's pointers.
P3VerifyArgs P3ProverDev::verify_args() const {
  const P3Shape& s = shape_;
  P3VerifyArgs a{};
  a.prog = prog_.instr.data();
  a.consts = prog_.consts.data();
  a.zfirst_inv = zfirst_inv_.data();
  a.k = s.k; a.B = s.B; a.L = s.L; a.Q = s.Q; a.W = s.W;
  a.num_queries = s.num_queries; a.pow_bits = s.pow_bits; a.n_instr = s.n_instr;
  a.num_inputs = (uint32_t)num_inputs();
  a.n_public = s.n_public;
  a.o_public = a.num_inputs - s.n_public;
  a.per_coef = s.per_coef;
  a.PW = s.PW;
  a.NC = s.NC;
  a.AW = s.AW;
  a.o_aux = s.o_aux;
  a.nb = 2 + (s.PW ? 1 : 0) + (s.AW ? 1 : 0);
  a.prep_root = prep_root_;   // the host's copy, known once a compute call has made it; verify_dev puts the device's in its place
  a.o_open = 8;
  a.o_roots = s.o_fri;
  a.o_qp = s.hdr_words;
  a.sz_a = s.sz_a;
  a.o_final = a.o_qp + s.num_queries * s.sz_a;
  a.o_pow = a.o_final + 2;
  a.o_qo = a.o_pow + 1;
  a.sz_b = s.sz_b;
  a.c_idx = P3VC_BETAS + 2 * s.k;
  a.c_chal = a.c_idx + s.num_queries;
  a.chal_stride = a.c_chal + (s.AW ? 2 * s.NC : 0);
  if ((size_t)a.o_qo + (size_t)s.num_queries * s.sz_b != a.o_public || a.o_roots + 4 * s.k != s.hdr_words ||
      p3v_round_off(a, s.k) != s.sz_a || (size_t)a.chal_stride + 2 * (size_t)s.num_queries * s.k != verify_scratch_words_per_proof())
    throw std::logic_error("p3 verifier: layout out of step with the proof's");
  a.w_L = s.w[s.L];
  a.w_L_inv = s.w_inv[s.L];
  a.w_n = s.w[s.k];
  a.g_inv = s.g_inv;
  a.neg2_inv = gl::inv(gl::neg(2));
  for (int i = 0; i < 8; i++) a.s_inv[i] = s.s_inv[i];
  return a;
}

void P3ProverDev::verify_dev(const u64* d_inputs, size_t n_proofs, size_t input_stride, uint32_t* d_status, hipStream_t st) {
  if (!n_proofs) return;
  ensure_impl();
  ensure_preprocessed(false, st);   // the 4 words of the preprocessed commitment: all this side needs of the columns
  P3VerifyArgs a = verify_args();
  a.stride = input_stride;
  a.prog = reinterpret_cast<const P3Instr*>(impl_->prog.p);
  a.consts = impl_->consts.p;
  a.zfirst_inv = impl_->zfirst.p;
  a.prep_root = impl_->prep_root.p;

  const size_t C = verify_chunk(n_proofs), per = verify_scratch_words_per_proof(), need = C * per;
  if (impl_->vscratch.words < need) {
    sync();   // an earlier call may still be using the old allocation
    impl_->vscratch.regrow(need);
  }
  // one buffer: wait, on the device, for the handle's call before, whichever stream it went to (also a proving call whose
  // proofs these may be); chunks follow each other on `st`
  if (impl_->recorded) P25_HIP(hipStreamWaitEvent(st, impl_->done, 0));
  P3CallRecord record{impl_, st};
  for (size_t c0 = 0; c0 < n_proofs; c0 += C) {
    const size_t cnt = std::min(C, n_proofs - c0);
    a.proofs = d_inputs + c0 * input_stride;
    a.n_proofs = (uint32_t)cnt;
    a.status = d_status + c0;
    a.chal = impl_->vscratch.p;
    a.folded = a.chal + cnt * a.chal_stride;
    launch_p3_verify(a, st);
  }
  P25_HIP(hipGetLastError());
}

void P3ProverDev::verify_host(const u64* inputs, size_t n_proofs, size_t input_stride, int32_t* statuses) {
  if (!n_proofs) return;
  const size_t ni = num_inputs();
  ensure_impl();
  hipStream_t st = impl_->host_stream();
  DevMem d_in(n_proofs * ni), d_status((n_proofs + 1) / 2);
  // the input_stride - num_inputs words behind a proof stay on the host: they are not read
  P25_HIP(hipMemcpy2DAsync(d_in.p, ni * 8, inputs, input_stride * 8, ni * 8, n_proofs, hipMemcpyHostToDevice, st));
  verify_dev(d_in.p, n_proofs, ni, reinterpret_cast<uint32_t*>(d_status.p), st);
  statuses_to_host(reinterpret_cast<const uint32_t*>(d_status.p), n_proofs, statuses, st);
}

}  // namespace p25
