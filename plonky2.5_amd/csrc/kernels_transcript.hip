// Device-resident Fiat-Shamir transcript and proof-of-work search.
//
// Replaces upstream plonky2 @ 3de92d9 iop/challenger.rs `Challenger<F, PoseidonHash>` and
// fri/prover.rs `fri_proof_of_work` (reached from /root/reference/src/p3/mod.rs:260).
// Semantics: duplex sponge, rate 8; `observe` buffers inputs and
// duplexes at 8; `get_challenge` duplexes if inputs are pending or no outputs remain, then pops
// from the END of the 8-word output buffer.  PoW: the smallest u64 witness w such that observing
// w and squeezing yields a challenge with >= pow_bits leading zero bits.
//
// The transcript is strictly sequential, so it is latency- not throughput-bound: one wavefront runs
// it, with sponge lane r living in wavefront lane r and the Poseidon permutation computed
// cooperatively -- S-boxes in parallel across 12 lanes, the circulant MDS layer as 12 cross-lane
// reads (ds_bpermute) + multiply-adds per lane.  That cuts a permutation's dependent chain from
// ~1.5k modular multiplies (one lane doing all 12 state words) to ~30 x (4 + MDS), i.e. a few us.
#include "kernels.h"
#include "coop.h"
#include "prover_kernels.h"

namespace p25 {

using coop::shfl64;

struct Sponge {
  u64 state, inb, outb;  // per-lane words (state: lanes 0..11, buffers: lanes 0..7)
  uint32_t n_in, n_out;  // wave-uniform
  int lane;
  const u64* rc;  // round constants in LDS
  __device__ void duplex() {
    if (lane < (int)n_in) state = inb;
    n_in = 0;
    state = coop::poseidon_permute_single(state, lane, rc);
    outb = state;
    n_out = 8;
  }
  __device__ void observe(u64 x) {
    n_out = 0;
    if (lane == (int)n_in) inb = x;
    n_in++;
    if (n_in == 8) duplex();
  }
  __device__ u64 challenge() {
    if (n_in > 0 || n_out == 0) duplex();
    u64 v = shfl64(outb, (int)n_out - 1);
    n_out--;
    return v;
  }
};

// One launch = one stretch of the challenger's script: reset (optional), observe up to TR_MAX_SEGMENTS segments in
// order, draw n_chal challenges, then one closing action (TranscriptArgs, prover_kernels.h).  A segment is loaded 64
// words at a time, one word per lane (which also stores it to copy_dst: how a Merkle cap, the final polynomial and the
// PoW witness reach the proof), and fed to the sponge from the lanes' registers; only the observe order is sequential.
__global__ __launch_bounds__(64) void k_transcript(Transcript* tr, TranscriptArgs a) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 rc_lds[360];
  coop::stage_poseidon_rc(rc_lds);
  const int lane = threadIdx.x;
  Sponge sp;
  sp.lane = lane;
  sp.rc = rc_lds;
  if (a.init) {
    sp.state = 0;
    sp.inb = 0;
    sp.outb = 0;
    sp.n_in = 0;
    sp.n_out = 0;
  } else {
    sp.state = lane < 12 ? tr->state[lane] : 0;
    sp.inb = lane < 8 ? tr->in[lane] : 0;
    sp.outb = lane < 8 ? tr->out[lane] : 0;
    sp.n_in = tr->n_in;
    sp.n_out = tr->n_out;
  }
  u64 w0 = 0;  // the first observed word (TR_CLOSE_FINISH: the PoW witness)
  for (uint32_t s = 0; s < a.n_seg; s++) {
    const TrSegment sg = a.seg[s];
    for (uint32_t base = 0; base < sg.n_words; base += 64) {
      const uint32_t cnt = sg.n_words - base < 64 ? sg.n_words - base : 64;
      u64 v = 0;
      if ((uint32_t)lane < cnt) {
        const uint32_t i = base + (uint32_t)lane;
        v = sg.src_b ? ((i & 1) ? sg.src_b : sg.src)[i >> 1] : sg.src[i];
        if (sg.copy_dst) sg.copy_dst[i] = v;
      }
      if (s == 0 && base == 0) w0 = shfl64(v, 0);
      for (uint32_t j = 0; j < cnt; j++) sp.observe(shfl64(v, (int)j));
    }
  }
  u64 c0 = 0, c1 = 0;  // the first two challenges, for the closing action
  for (uint32_t i = 0; i < a.n_chal; i++) {
    u64 c = sp.challenge();
    if (i == 0) c0 = c;
    if (i == 1) c1 = c;
    if (lane == 0) a.chal_out[i] = c;
  }
  if (lane < 12) tr->state[lane] = sp.state;
  if (lane < 8) {
    tr->in[lane] = sp.inb;
    tr->out[lane] = sp.outb;
  }
  if (lane == 0) {
    tr->n_in = sp.n_in;
    tr->n_out = sp.n_out;
  }
  switch (a.close) {
    case TR_CLOSE_ALPHA_POWS: {  // (c0, c1) = alphas: out[c][j] = alpha_c^j, j < ALPHA_POWS; lane l takes j = l (mod 64)
      for (int c = 0; c < 2; c++) {
        const u64 al = c ? c1 : c0, al64 = gl::pow(al, 64);
        u64 p = gl::pow(al, (u64)lane);
        for (int j = lane; j < ALPHA_POWS; j += 64) {
          a.close_out[c * ALPHA_POWS + j] = p;
          p = gl::mul(p, al64);
        }
      }
      break;
    }
    case TR_CLOSE_CHECK_ZETA: {  // (c0, c1) = zeta
      gl::E2 zn = gl::exp_pow2(gl::E2{c0, c1}, a.close_arg);
      if (lane == 0 && zn.a == 1 && zn.b == 0) set_status(a.status, 6);  // "Opening point is in the subgroup."
      break;
    }
    case TR_CLOSE_POW_INIT:
      if (lane == 0) *a.close_out = ~0ull;
      break;
    case TR_CLOSE_FINISH:  // w0 = the witness just observed (none found: ~0), c0 = the PoW response
      if (lane == 0 && (w0 == ~0ull || (uint32_t)__clzll((long long)c0) < a.close_arg)) set_status(a.status, 7);
      break;
    default:
      break;
  }
}

void launch_transcript(Transcript* d_tr, const TranscriptArgs& a, hipStream_t st) {
  if (a.n_seg > TR_MAX_SEGMENTS) throw std::invalid_argument("too many transcript segments in one launch");
  hipLaunchKernelGGL(k_transcript, dim3(1), dim3(64), 0, st, d_tr, a);
}
void launch_transcript(Transcript* d_tr, int init, const u64* d_obs, uint32_t n_obs, u64* d_chal_out,
                       uint32_t n_chal, hipStream_t st) {
  TranscriptArgs a{};
  a.seg[0] = TrSegment{d_obs, nullptr, nullptr, n_obs};
  a.n_seg = 1;
  a.init = (uint32_t)init;
  a.chal_out = d_chal_out;
  a.n_chal = n_chal;
  launch_transcript(d_tr, a, st);
}

// The PoW search in one launch: lane t tries the candidates t, t + G, t + 2G, ... (G = the grid's lane count) in
// increasing order and leaves as soon as a witness below its next candidate is known.  A lane only ever skips
// candidates above a witness already found, so *result ends as the smallest witness among the first `total` candidates
// (~0, as the launch before left it, if there is none).  No lane waits for another.
// PRIO: the wave priority, chosen per launch by launch_pow_search.
template <int PRIO>
__global__ __launch_bounds__(256) void k_pow_search(const Transcript* __restrict__ tr, uint32_t pow_bits, u64 total,
                                                    u64* result) {
  if constexpr (PRIO != 0) P25_WAVE_PRIO(PRIO);
  const u64 G = (u64)gridDim.x * blockDim.x;
  for (u64 cand = (u64)blockIdx.x * blockDim.x + threadIdx.x; cand < total; cand += G) {
    if (__hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < cand) return;
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = tr->state[i];
    const uint32_t pos = tr->n_in;
    for (uint32_t i = 0; i < pos; i++) s[i] = tr->in[i];
    // witness goes to sponge position `pos` (an invariant of the challenger: pos < 8)
#pragma unroll
    for (int i = 0; i < 8; i++)
      if ((uint32_t)i == pos) s[i] = cand;
    poseidon::permute(s);
    // No `return` after the atomicMin: the compiler would sink the atomic below the loop, where a wave only arrives once
    // ALL its lanes have left, i.e. after the other lanes have run out of candidates.  The finder leaves at its next check.
    if ((uint32_t)__clzll((long long)s[7]) >= pow_bits) atomicMin((unsigned long long*)result, (unsigned long long)cand);
  }
}

// hash_no_pad of a proof's public inputs (overwrite-mode sponge, rate 8; hash/hashing.rs `hash_n_to_m_no_pad`): state
// word r in lane r, one cooperative permutation per chunk of 8.
__global__ __launch_bounds__(64) void k_public_inputs(const u64* __restrict__ vals, size_t B, uint32_t p,
                                                      const uint32_t* __restrict__ pi_slots, uint32_t n,
                                                      u64* __restrict__ values_out, u64* __restrict__ hash_out) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 rc_lds[360];
  coop::stage_poseidon_rc(rc_lds);
  const int lane = threadIdx.x;
  u64 s = 0;
  for (uint32_t off = 0; off < n; off += 8) {
    if (lane < 8 && off + lane < n) {
      s = vals[(size_t)pi_slots[off + lane] * B + p];
      values_out[off + lane] = s;
    }
    s = coop::poseidon_permute_single(s, lane, rc_lds);
  }
  if (lane < 4) hash_out[lane] = s;
}
void launch_public_inputs(const u64* d_vals, size_t B, uint32_t p, const uint32_t* d_pi_slots, uint32_t n, u64* d_values_out,
                          u64* d_hash_out, hipStream_t st) {
  hipLaunchKernelGGL(k_public_inputs, dim3(1), dim3(64), 0, st, d_vals, B, p, d_pi_slots, n, d_values_out, d_hash_out);
}

// Wave priority of the search when many proofs are in flight (= LEVEL_PRIO_BATCH, kernels_hash.hip, and for its reason):
// one or two sweeps of a single permutation per lane, a wave per SIMD, which at priority 0 beside the other queues'
// leaf sponges took 631 us in the pipeline against 86 us alone (profiles/r07_fused_chain.txt section 4b) while the three
// other proofs of its in-order queue waited.  Measured: profiles/r09_fri_pow_queue_time.txt.  A lone proof has no other
// proof's sponge beside it and keeps priority 0.
constexpr int POW_PRIO_BATCH = 1;
void launch_pow_search(const Transcript* d_tr, int pow_bits, u64* d_result, hipStream_t st, bool single_proof) {
  // *d_result = ~0 comes from the transcript launch that observed the final polynomial (TR_CLOSE_POW_INIT).
  // Expected number of candidates is 2^pow_bits.  The grid is 2^16 lanes (2^12 for pow_bits <= 12), so the expected
  // work is ~1.6 x 2^pow_bits permutations; the search gives up after 2^(pow_bits + 6) candidates, which happens with
  // probability e^-64 (reported as P25_ERR_INTERNAL by the transcript launch that observes the witness).
  const int wb = pow_bits < 12 ? 12 : pow_bits;
  const int gb = wb < 16 ? wb : 16;
  const dim3 grid(1u << (gb - 8));
  const u64 total = (u64)1 << (wb + 6);
  if (single_proof)
    hipLaunchKernelGGL(k_pow_search<0>, grid, dim3(256), 0, st, d_tr, (uint32_t)pow_bits, total, d_result);
  else
    hipLaunchKernelGGL(k_pow_search<POW_PRIO_BATCH>, grid, dim3(256), 0, st, d_tr, (uint32_t)pow_bits, total, d_result);
}

}  // namespace p25
