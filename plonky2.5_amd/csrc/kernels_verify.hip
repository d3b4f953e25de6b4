// The batch verifier: upstream plonky2 @ 3de92d9 `verify` (plonk/verifier.rs `verify_with_challenges`, fri/verifier.rs
// `verify_fri_proof`), which the reference reaches through `data.verify(proof)` (`src/p3/mod.rs:266` of the reference).
//
// The verifier is the prover in reverse and tiny next to it (~3.5 k permutations per fib-64 proof against 13.4 M), so
// one proof cannot fill the device: every stage below is ONE launch over the whole batch (thin
// launches), with the batch as the source of parallelism.
//   k_verify_transcript  the challenger's script replayed from the proof: a chain of ~130 dependent permutations, run on
//                        the cooperative 16-lane permutation of coop.h, four proofs per wave; the same lanes scan the
//                        proof for words >= p first
//   k_verify_vanishing   the constraint check at zeta in F_p^2 (ext_gates.h): lane = (gate type or permutation argument
//                        of one challenge, proof), task-major so that a wave runs one gate kind on 64 proofs
//   k_verify_fri         lane = (Merkle tree or the query's arithmetic, proof, query): the hashing lanes run the per-lane
//                        Poseidon of poseidon.h through one call site per path step
//   k_verify_verdict     per proof: folds the vanishing partials, checks the identity and the PoW, decodes the key
// Checks that run in parallel report through atomicMin on a key ordered like the sequential verifier (verify_kernels.h).
// All arithmetic is canonical (gl::, extf::): a proof with a word >= p is rejected by the scan, whatever the later
// stages make of it -- they only have to stay inside the proof, which they do (every index is derived from the layout
// and a query index is masked to the LDE domain).
#include "coop.h"
#include "verify_lanes.h"

namespace p25 {

using coop::shfl64;

namespace {

// The duplex sponge of kernels_transcript.hip for one 16-lane group: state word r in lane r of the group.  The script
// (how many words, how many challenges) is the same for every proof of a circuit, so the counters are wave-uniform.
struct GroupSponge {
  u64 state, inb, outb;
  uint32_t n_in, n_out;
  int lane, rr, base;
  const u64* rc;
  __device__ void duplex() {
    if (rr < (int)n_in) state = inb;
    n_in = 0;
    state = coop::poseidon_permute(state, lane, rc);
    outb = state;
    n_out = 8;
  }
  __device__ void observe(u64 x) {  // x: the same in every lane of the group
    n_out = 0;
    if (rr == (int)n_in) inb = x;
    n_in++;
    if (n_in == 8) duplex();
  }
  __device__ u64 challenge() {
    if (n_in > 0 || n_out == 0) duplex();
    const u64 v = shfl64(outb, base + (int)n_out - 1);
    n_out--;
    return v;
  }
  __device__ void observe_words(const u64* src, uint32_t n) {
    for (uint32_t b = 0; b < n; b += coop::GROUP) {
      const uint32_t cnt = n - b < (uint32_t)coop::GROUP ? n - b : (uint32_t)coop::GROUP;
      const u64 v = (uint32_t)rr < cnt ? src[b + rr] : 0;
      for (uint32_t j = 0; j < cnt; j++) observe(shfl64(v, base + (int)j));
    }
  }
};

}  // namespace

constexpr int PROOFS_PER_WAVE = 64 / coop::GROUP;

__global__ __launch_bounds__(64) void k_verify_transcript(VerifyArgs a) {
  __shared__ u64 rc[360];
  coop::stage_poseidon_rc(rc);
  const int lane = threadIdx.x, rr = lane & (coop::GROUP - 1), base = lane & ~(coop::GROUP - 1);
  uint32_t p = blockIdx.x * PROOFS_PER_WAVE + (uint32_t)(lane / coop::GROUP);
  const bool live = p < a.n_proofs;   // a group past the batch replays the last proof and stores nothing:
  if (!live) p = a.n_proofs - 1;      // the shuffles of the cooperative permutation want the whole wave
  const u64* proof = a.proofs + (size_t)p * a.stride;
  u64* chal = a.chal + (size_t)p * VCH_WORDS;

  uint32_t bad = 0;
  for (uint32_t i = (uint32_t)rr; i < a.proof_words; i += coop::GROUP) bad |= proof[i] >= gl::P ? 1u : 0u;
  for (int m = 1; m < coop::GROUP; m <<= 1) bad |= (uint32_t)__shfl_xor((int)bad, m);
  if (live && rr == 0) a.status[p] = bad ? (uint32_t)VKEY_MALFORMED : (uint32_t)VKEY_NONE;

  // hash_no_pad(public_inputs): overwrite-mode sponge, words 0..3 of the state end in lanes 0..3 of the group
  u64 pih = 0;
  for (uint32_t off = 0; off < a.num_public_inputs; off += 8) {
    if (rr < 8 && off + rr < a.num_public_inputs) pih = proof[a.public_inputs + off + rr];
    pih = coop::poseidon_permute(pih, lane, rc);
  }
  if (live && rr < 4) chal[VCH_PI_HASH + rr] = pih;

  GroupSponge sp;
  sp.state = sp.inb = sp.outb = 0;
  sp.n_in = sp.n_out = 0;
  sp.lane = lane;
  sp.rr = rr;
  sp.base = base;
  sp.rc = rc;
  auto draw = [&](uint32_t slot, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
      const u64 c = sp.challenge();
      if (live && rr == 0) chal[slot + i] = c;
    }
  };
  sp.observe_words(a.digest, 4);
  for (int j = 0; j < 4; j++) sp.observe(shfl64(pih, base + j));
  sp.observe_words(proof + a.wires_cap, a.cap_words);
  draw(CH_BETAS, 2);
  draw(CH_GAMMAS, 2);
  sp.observe_words(proof + a.zs_cap, a.cap_words);
  draw(CH_ALPHAS, 2);
  sp.observe_words(proof + a.quotient_cap, a.cap_words);
  draw(CH_ZETA, 2);
  // openings in the challenger's order: constants | sigmas | wires | zs | partial products | quotient, then zs_next
  // (the flat layout keeps zs_next behind zs)
  sp.observe_words(proof + a.constants, a.zs_next - a.constants);
  sp.observe_words(proof + a.pps, a.fri_caps - a.pps);
  sp.observe_words(proof + a.zs_next, a.pps - a.zs_next);
  draw(CH_FRI_ALPHA, 2);
  for (uint32_t l = 0; l < a.n_layers; l++) {
    sp.observe_words(proof + a.fri_caps + l * a.cap_words, a.cap_words);
    draw(CH_FRI_BETAS + 2 * l, 2);
  }
  sp.observe_words(proof + a.final_poly, 2 * a.final_poly_len);
  sp.observe_words(proof + a.pow_witness, 1);
  if (live && rr == 0) chal[CH_POW_WITNESS] = proof[a.pow_witness];
  draw(CH_POW_RESPONSE, 1);
  draw(CH_QUERIES, a.num_queries);
}

__global__ __launch_bounds__(64) void k_verify_vanishing(VerifyArgs a) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)(a.n_gates + 2) * a.n_proofs) return;
  vlane::vanishing_lane(a, (uint32_t)(gid / a.n_proofs), (uint32_t)(gid % a.n_proofs));   // task-major
}

__global__ __launch_bounds__(64) void k_verify_fri(VerifyArgs a) {
  const size_t per_task = (size_t)a.n_proofs * a.num_queries;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= per_task * (5 + a.n_layers)) return;
  const uint32_t p = (uint32_t)((gid % per_task) / a.num_queries);
  const uint32_t key = vlane::fri_lane(a, (uint32_t)(gid / per_task), p, (uint32_t)(gid % a.num_queries));
  if (key != VKEY_NONE) atomicMin(a.status + p, key);
}

__global__ __launch_bounds__(64) void k_verify_verdict(VerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < a.n_proofs) a.status[p] = vlane::verdict_lane(a, p, a.status[p]);
}

static uint32_t blocks_of(size_t lanes, uint32_t block) { return (uint32_t)((lanes + block - 1) / block); }

void launch_verify_transcript(const VerifyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_transcript, dim3(blocks_of(a.n_proofs, PROOFS_PER_WAVE)), dim3(64), 0, st, a);
}
void launch_verify_vanishing(const VerifyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_vanishing, dim3(blocks_of((size_t)(a.n_gates + 2) * a.n_proofs, 64)), dim3(64), 0, st, a);
}
void launch_verify_fri(const VerifyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_fri, dim3(blocks_of((size_t)a.n_proofs * a.num_queries * (5 + a.n_layers), 64)), dim3(64), 0, st, a);
}
void launch_verify_verdict(const VerifyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_verdict, dim3(blocks_of(a.n_proofs, 64)), dim3(64), 0, st, a);
}

}  // namespace p25
