// The plonky3 batch verifier: src/p3/verifier.rs, which the reference states only as a circuit, run natively on the flat
// proofs that p25_p3_prove_batch writes and p25_prove_batch reads.
//
// As for the outer verifier (kernels_verify.hip) one proof is a short dependent chain followed by num_queries x (2 + k)
// independent Merkle paths, far too little to fill the device: every stage is ONE launch over the whole batch.
//   k_p3v_transcript  the duplex challenger replayed from the proof on the cooperative 16-lane Poseidon2 of coop.h, four
//                     proofs per wave; the same lanes scan the proof for words >= p first
//   k_p3v_identity    lane = proof: the quotient identity at zeta in F_p^2 with the handle's AIR program (run_air)
//   k_p3v_fold        lane = (proof, query): reduced opening and fold chain, the value of every round to scratch
//   k_p3v_merkle      lane = (tree, proof, query), task-major: a wave runs ONE tree kind on 64 (proof, query) pairs, so
//                     its lanes walk paths of one depth through one permutation call site
//   k_p3v_verdict     lane = proof: key -> code
// Checks that run in parallel report through atomicMin on a key ordered like the sequential verifier (p3_verify_lanes.h).
// All arithmetic is canonical: a proof with a word >= p is rejected by the scan, whatever the later stages make of it --
// they only have to stay inside the proof, which they do (every offset comes from the shape and a query index is masked
// to the LDE domain).
#include "coop.h"
#include "p3_verify_lanes.h"

namespace p25 {

using coop::shfl64;

namespace {

struct NoEmit {
  __device__ void operator()(int, u64) const {}
};

// The challenger of p3vlane::Challenger for one 16-lane group: word r of the state and of both buffers in lane r of the
// group.  The script is the same for every proof of a shape, so the counters are wave-uniform.
struct GroupChallenger {
  u64 st, inb, outb;
  uint32_t n_in, n_out;
  int lane, rr, base;
  const u64* rc;
  __device__ void duplex() {
    if (rr < (int)n_in) st = inb;
    n_in = 0;
    st = coop::poseidon2_permute(st, lane, rc, NoEmit());
    outb = st;
    n_out = 12;
  }
  __device__ void observe(u64 x) {  // x: the same in every lane of the group
    n_out = 0;
    if (rr == (int)n_in) inb = x;
    n_in++;
    if (n_in == 12) duplex();
  }
  __device__ u64 sample() {
    if (n_in > 0 || n_out == 0) duplex();
    const u64 v = shfl64(outb, base + (int)n_out - 1);
    n_out--;
    return v;
  }
  // observes the 4 words at `d` (read by lanes 0..3 of the group)
  __device__ void observe_digest(const u64* d) {
    const u64 v = rr < 4 ? d[rr] : 0;
    for (int j = 0; j < 4; j++) observe(shfl64(v, base + j));
  }
};

constexpr int PROOFS_PER_WAVE = 64 / coop::GROUP;

}  // namespace

__global__ __launch_bounds__(64) void k_p3v_transcript(P3VerifyArgs a) {
  __shared__ u64 rc[coop::P2_LDS_WORDS];
  coop::stage_poseidon2_rc(rc);
  const int lane = threadIdx.x, rr = lane & (coop::GROUP - 1), base = lane & ~(coop::GROUP - 1);
  uint32_t p = blockIdx.x * PROOFS_PER_WAVE + (uint32_t)(lane / coop::GROUP);
  const bool live = p < a.n_proofs;   // a group past the batch replays the last proof and stores nothing:
  if (!live) p = a.n_proofs - 1;      // the shuffles of the cooperative permutation want the whole wave
  const u64* proof = a.proofs + (size_t)p * a.stride;
  u64* chal = a.chal + (size_t)p * a.chal_stride;

  uint32_t bad = 0;
  for (uint32_t i = (uint32_t)rr; i < a.num_inputs; i += coop::GROUP) bad |= proof[i] >= gl::P ? 1u : 0u;
  for (int m = 1; m < coop::GROUP; m <<= 1) bad |= (uint32_t)__shfl_xor((int)bad, m);

  GroupChallenger ch;
  ch.st = ch.inb = ch.outb = 0;
  ch.n_in = ch.n_out = 0;
  ch.lane = lane;
  ch.rr = rr;
  ch.base = base;
  ch.rc = rc;
  auto draw = [&](uint32_t slot, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
      const u64 c = ch.sample();
      if (live && rr == 0) chal[slot + i] = c;
    }
  };
  ch.observe_digest(proof);
  if (a.PW)   // the handle's preprocessed commitment: one address for the whole grid
    for (int j = 0; j < 4; j++) ch.observe(a.prep_root[j]);
  for (uint32_t i = 0; i < a.n_public; i++) ch.observe(proof[a.o_public + i]);   // one address per group: the value is uniform in it
  if (a.AW) {   // the challenge phase: the challenges, then the proof's auxiliary root, before alpha
    draw(a.c_chal, 2 * a.NC);
    ch.observe_digest(proof + a.o_aux);
  }
  draw(P3VC_ALPHA, 2);
  ch.observe_digest(proof + 4);
  draw(P3VC_ZETA, 2);
  draw(P3VC_FRI_ALPHA, 2);
  for (uint32_t r = 0; r < a.k; r++) {
    ch.observe_digest(proof + a.o_roots + 4 * r);
    draw(P3VC_BETAS + 2 * r, 2);
  }
  ch.observe(proof[a.o_pow]);
  const u64 resp = ch.sample() & (((u64)1 << a.pow_bits) - 1);
  for (uint32_t q = 0; q < a.num_queries; q++) {
    const u64 v = ch.sample() & (((u64)1 << a.L) - 1);
    if (live && rr == 0) chal[a.c_idx + q] = v;
  }
  if (live && rr == 0) {
    chal[P3VC_POW] = resp;
    chal[P3VC_POW + 1] = 0;
    a.status[p] = bad ? (uint32_t)P3VKEY_MALFORMED : resp != 0 ? (uint32_t)P3VKEY_POW : (uint32_t)P3VKEY_NONE;
  }
}

__global__ __launch_bounds__(64) void k_p3v_identity(P3VerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n_proofs) return;
  if (!p3vlane::identity_lane(a, p)) atomicMin(a.status + p, p3v_key_constraints(a));
}

__global__ __launch_bounds__(64) void k_p3v_fold(P3VerifyArgs a) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)a.n_proofs * a.num_queries) return;
  const uint32_t p = (uint32_t)(gid / a.num_queries);
  const uint32_t key = p3vlane::fold_lane(a, p, (uint32_t)(gid % a.num_queries));
  if (key != P3VKEY_NONE) atomicMin(a.status + p, key);
}

// Five waves per SIMD stated, not left to the scheduler: with the third tree kind in the lane function it settles on 112
// registers (four waves) unasked, and on the 93 it took before (no scratch) when asked.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void k_p3v_merkle(P3VerifyArgs a) {
  const size_t per_tree = (size_t)a.n_proofs * a.num_queries;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= per_tree * (a.nb + a.k)) return;
  const uint32_t p = (uint32_t)((gid % per_tree) / a.num_queries);
  const uint32_t key = p3vlane::merkle_lane(a, (uint32_t)(gid / per_tree), p, (uint32_t)(gid % a.num_queries));   // task-major
  if (key != P3VKEY_NONE) atomicMin(a.status + p, key);
}

__global__ __launch_bounds__(64) void k_p3v_verdict(P3VerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < a.n_proofs) a.status[p] = p3vlane::verdict_lane(a, a.status[p]);
}

static uint32_t blocks_of(size_t lanes, uint32_t block) { return (uint32_t)((lanes + block - 1) / block); }

void launch_p3_verify(const P3VerifyArgs& a, hipStream_t st) {
  const size_t pq = (size_t)a.n_proofs * a.num_queries;
  hipLaunchKernelGGL(k_p3v_transcript, dim3(blocks_of(a.n_proofs, PROOFS_PER_WAVE)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_p3v_identity, dim3(blocks_of(a.n_proofs, 64)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_p3v_fold, dim3(blocks_of(pq, 64)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_p3v_merkle, dim3(blocks_of(pq * (a.nb + a.k), 64)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_p3v_verdict, dim3(blocks_of(a.n_proofs, 64)), dim3(64), 0, st, a);
}

}  // namespace p25
