// The plonky3 prover's stages on the device: Poseidon2 MMCS, duplex challenger, AIR quotient, openings, two-adic FRI,
// proof of work and the query gather.  Every kernel takes the proofs of a group as blockIdx.y.
//
// Replaces the host function p3_prove_air (p3_prover.cpp), stage for stage and word for word; that function restates the
// prover whose proofs the reference ships as artifacts/proof_fibonacci.json (data model src/p3/serde/proof.rs:349-383) and
// whose verifier is src/p3/verifier.rs:
//   MMCS hash / compress   src/p3/commit.rs:23-60        (k_p3_leaf_*, k_p3_tree_*)
//   challenger             src/p3/challenger.rs:70-169   (Chal, k_p3_chain)
//   selectors, domains     src/p3/serde/two_adic.rs:100-147, verifier.rs:120-124 (k_p3_quotient)
//   identity at zeta       src/p3/verifier.rs:169-239    (k_p3_identity)
//   reduced openings       src/p3/verifier.rs:296-338    (k_p3_reduced)
//   FRI fold               src/p3/verifier.rs:441-516    (k_p3_fold, k_p3_fri_tail)
// Field arithmetic is exact, so any evaluation order gives the host's words; the orders the protocol fixes (constraint
// fold, transcript, flattening) are the host's.
#include "coop.h"
#include "p3_air_run.h"

namespace p25 {
namespace {
using gl::E2;

struct NoEmit {
  __device__ void operator()(int, u64) const {}
};
__device__ __forceinline__ u64 coop_p2(u64 s, int lane, const u64* rc) { return coop::poseidon2_permute(s, lane, rc, NoEmit()); }

__device__ __forceinline__ E2 ld_e2(const u64* p) { return E2{p[0], p[1]}; }
__device__ __forceinline__ void st_e2(u64* p, E2 v) {
  p[0] = v.a;
  p[1] = v.b;
}

// ---------------------------------------------------------------------------------------------------------------------
// MMCS
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_p3_transpose(const u64* __restrict__ traces, size_t trace_stride, u64* __restrict__ cols,
                                                      uint32_t W, uint32_t log_n) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  const size_t n = (size_t)1 << log_n, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * W) return;
  const size_t r = e / W, c = e % W;
  cols[((size_t)blockIdx.y * W + c) * n + r] = traces[(size_t)blockIdx.y * trace_stride + e];
}

// hash_row (commit.rs:23-60): one lane per row, ceil(width / 4) permutations, each overwriting the first words of the state
__global__ __launch_bounds__(256) void k_p3_leaf_cols(const u64* __restrict__ base, size_t proof_stride, size_t pair_stride,
                                                      size_t col_stride, uint32_t width, size_t h, u64* __restrict__ tree,
                                                      size_t tree_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const u64* m = base + (size_t)blockIdx.y * proof_stride + i;
  u64 s[12] = {0};
  for (uint32_t off = 0; off < width; off += 4) {
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t c = off + j;
      if (c < width) s[j] = m[(size_t)(c >> 1) * pair_stride + (size_t)(c & 1) * col_stride];
    }
    poseidon2::permute(s);
  }
  u64* d = tree + (size_t)blockIdx.y * tree_stride + 4 * i;
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = s[j];
}
__global__ __launch_bounds__(256) void k_p3_leaf_rows4(const u64* __restrict__ rows, size_t rows_stride, size_t h,
                                                       u64* __restrict__ tree, size_t tree_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const u64* m = rows + (size_t)blockIdx.y * rows_stride + 4 * i;
  u64 s[12] = {0};
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = m[j];
  poseidon2::permute(s);
  u64* d = tree + (size_t)blockIdx.y * tree_stride + 4 * i;
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = s[j];
}
// compress (commit.rs): one lane per node of a large level
__global__ __launch_bounds__(256) void k_p3_tree_level(const u64* __restrict__ in, u64* __restrict__ out, size_t nodes,
                                                       size_t tree_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nodes) return;
  const u64* m = in + (size_t)blockIdx.y * tree_stride + 8 * i;
  u64 s[12] = {0};
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = m[j];
  poseidon2::permute(s);
  u64* d = out + (size_t)blockIdx.y * tree_stride + 4 * i;
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = s[j];
}
// one level with a 16-lane group per node (group `gid` of `ngroups`)
__device__ __forceinline__ void coop_level(const u64* in, u64* out, size_t nodes, uint32_t gid, uint32_t ngroups, int lane,
                                           const u64* rc) {
  const int rr = lane & 15;
  for (size_t i = gid; i < nodes; i += ngroups) {
    u64 s = rr < 8 ? in[8 * i + rr] : 0;
    s = coop_p2(s, lane, rc);
    if (rr < 4) out[4 * i + rr] = s;
  }
}
// Small levels, 16 lanes per node.  One level over the whole grid (n_levels = 1), or, for the top of the tree, the remaining
// levels of each proof in one workgroup.
__global__ __launch_bounds__(256) void k_p3_tree_coop(u64* __restrict__ tree, size_t tree_stride, size_t h, uint32_t level,
                                                      uint32_t n_levels) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 rc[coop::P2_LDS_WORDS];
  coop::stage_poseidon2_rc(rc);
  u64* t = tree + (size_t)blockIdx.y * tree_stride;
  const uint32_t gid = blockIdx.x * 16 + (threadIdx.x >> 4), ngroups = gridDim.x * 16;
  for (uint32_t l = level; l < level + n_levels; l++) {
    coop_level(t + p3_level_off(h, l), t + p3_level_off(h, l + 1), h >> (l + 1), gid, ngroups, threadIdx.x & 63, rc);
    if (n_levels > 1) __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Challenger: state word r in lane r of the wave, the permutation by the wave's first 16-lane group
// ---------------------------------------------------------------------------------------------------------------------
struct Chal {
  u64 st, inb, outb;
  uint32_t n_in, n_out;
  int lane;
  const u64* rc;
  __device__ void load(const P3State* s) {
    st = lane < 12 ? s->st[lane] : 0;
    inb = lane < 12 ? s->inb[lane] : 0;
    outb = lane < 12 ? s->outb[lane] : 0;
    n_in = s->n_in;
    n_out = s->n_out;
  }
  __device__ void store(P3State* s) const {
    if (lane < 12) {
      s->st[lane] = st;
      s->inb[lane] = inb;
      s->outb[lane] = outb;
    }
    if (lane == 0) {
      s->n_in = n_in;
      s->n_out = n_out;
    }
  }
  __device__ void duplex() {
    if (lane < (int)n_in) st = inb;
    n_in = 0;
    st = coop_p2(st, lane, rc);
    outb = st;
    n_out = 12;
  }
  __device__ void observe(u64 x) {
    n_out = 0;
    if (lane == (int)n_in) inb = x;
    n_in++;
    if (n_in == 12) duplex();
  }
  __device__ u64 sample() {
    if (n_in > 0 || n_out == 0) duplex();
    const u64 v = coop::shfl64(outb, (int)n_out - 1);
    n_out--;
    return v;
  }
  // observes the 4 words at `d` (read by lanes 0..3)
  __device__ void observe_digest(const u64* d) {
    const u64 v = lane < 4 ? d[lane] : 0;
    for (int j = 0; j < 4; j++) observe(coop::shfl64(v, j));
  }
  __device__ E2 sample_ext() {
    const u64 a = sample();
    const u64 b = sample();
    return E2{a, b};
  }
};

__device__ __forceinline__ void set_p3_status(P3State* s, uint32_t code) { atomicCAS(&s->status, 0u, code); }

__global__ __launch_bounds__(64) void k_p3_chain(P3Shape sh, P3Bufs b, uint32_t phase, uint32_t round) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 rc[coop::P2_LDS_WORDS];
  coop::stage_poseidon2_rc(rc);
  const int lane = threadIdx.x;
  const uint32_t g = blockIdx.y;
  const size_t N2 = (size_t)1 << sh.L;
  P3State* s = b.state + g;
  u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  Chal ch;
  ch.lane = lane;
  ch.rc = rc;
  if (phase == P3_CH_TRACE) {
    ch.st = ch.inb = ch.outb = 0;
    ch.n_in = ch.n_out = 0;
    if (lane == 0) {
      s->status = 0;
      s->pow_witness = ~0ull;
    }
  } else {
    ch.load(s);
  }
  switch (phase) {
    case P3_CH_TRACE:
    case P3_CH_QUOTIENT: {
      const u64* root = (phase == P3_CH_TRACE ? b.ttree : b.qtree) + (size_t)g * 8 * N2 + p3_level_off(N2, sh.L);
      u64* dst = hdr + 4 * phase;
      if (lane < 4) dst[lane] = root[lane];
      ch.observe_digest(root);
      // the preprocessed commitment (the handle's shared tree: no group offset), directly behind the trace root
      if (phase == P3_CH_TRACE && sh.PW) ch.observe_digest(b.ptree + p3_level_off(N2, sh.L));
      if (phase == P3_CH_TRACE) {   // the proof's public values, between the trace root and alpha (p3_prover.cpp)
        const u64* pub = b.pub + (size_t)g * sh.n_public;
        for (uint32_t i = 0; i < sh.n_public; i++) ch.observe(pub[i]);
        if (sh.AW) {   // the challenge phase: the challenges to the header; alpha waits for the auxiliary root (P3_CH_AUX)
          for (uint32_t i = 0; i < sh.NC; i++) {
            const E2 c = ch.sample_ext();
            if (lane == 0) st_e2(hdr + sh.o_chal + 2 * i, c);
          }
          break;
        }
      }
      const E2 c = ch.sample_ext();
      if (lane == 0) {
        if (phase == P3_CH_TRACE) {
          st_e2(s->alpha, c);
        } else {
          st_e2(s->zeta, c);
          u64* pts = hdr + sh.o_points;
          st_e2(pts, c);
          st_e2(pts + 2, gl::mul(c, sh.w[sh.k]));
          for (uint32_t q = 0; q < sh.Q; q++) st_e2(pts + 4 + 2 * q, gl::mul(c, sh.s_inv[q]));
        }
      }
      break;
    }
    case P3_CH_AUX: {   // the auxiliary root: to the header, observed, then alpha
      const u64* root = b.atree + (size_t)g * 8 * N2 + p3_level_off(N2, sh.L);
      u64* dst = hdr + sh.o_aux;
      if (lane < 4) dst[lane] = root[lane];
      ch.observe_digest(root);
      const E2 c = ch.sample_ext();
      if (lane == 0) st_e2(s->alpha, c);
      break;
    }
    case P3_CH_FRI_ALPHA: {
      const E2 fa = ch.sample_ext();
      if (lane == 0) {
        st_e2(s->fri_alpha, fa);
        u64* ap = hdr + sh.o_apow;
        E2 p = gl::e2(1);
        for (uint32_t i = 0; i < 2 * sh.W + 2 * sh.Q + 2 * sh.PW + 4 * sh.AW; i++) {
          st_e2(ap + 2 * i, p);
          p = gl::mul(p, fa);
        }
      }
      break;
    }
    case P3_CH_FRI_ROUND: {
      const size_t h = N2 >> (round + 1);
      const u64* root = b.ftrees + (size_t)g * 8 * N2 + p3_ftree_off(N2, round) + p3_level_off(h, sh.L - round - 1);
      u64* dst = hdr + sh.o_fri + 4 * round;
      if (lane < 4) dst[lane] = root[lane];
      ch.observe_digest(root);
      const E2 beta = ch.sample_ext();
      if (lane == 0) st_e2(hdr + sh.o_betas + 2 * round, beta);
      break;
    }
    default: {  // P3_CH_QUERIES: challenger.rs:159-168, then the query indices
      u64 wit = s->pow_witness;
      if (wit == ~0ull) {
        if (lane == 0) set_p3_status(s, 7);
        wit = 0;
      }
      ch.observe(wit);
      const u64 resp = ch.sample() & (((u64)1 << sh.pow_bits) - 1);
      if (resp != 0 && lane == 0) set_p3_status(s, 7);
      uint32_t* idx = reinterpret_cast<uint32_t*>(hdr + sh.o_idx);
      for (uint32_t q = 0; q < sh.num_queries; q++) {
        const u64 v = ch.sample() & (((u64)1 << sh.L) - 1);
        if (lane == 0) idx[q] = (uint32_t)v;
      }
      break;
    }
  }
  ch.store(s);
}

// ---------------------------------------------------------------------------------------------------------------------
// The AIR program (run_air: p3_air_run.h)
// ---------------------------------------------------------------------------------------------------------------------
// The auxiliary columns' terms (include/p25.h "AUXILIARY COLUMNS"): one lane per (row, proof) runs the terms' program in
// ExtF on the trace VALUES (natural order, next = (i + 1) mod n; the preprocessed columns' values from the handle, a
// periodic column by row mod P), inverts the row's denominators with ONE F_p^2 inversion (Montgomery's trick over
// AW <= 16) and writes t_j(i) = num_j / den_j component-split to tmp[g][2 j + component][i], where the scan takes it.  A
// zero denominator fails the proof like a failed identity; its terms are zeros.
__global__ __launch_bounds__(256) void k_p3_aux_terms(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  const size_t n = (size_t)1 << sh.k, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = blockIdx.y, AW = sh.AW;
  const size_t i1 = (i + 1) & (n - 1);
  const u64* tv = b.tvals + (size_t)g * sh.W * n;
  auto load = [&](int which, uint32_t c) -> E2 {
    return gl::e2(((which & 2) ? b.pvals : tv)[(size_t)c * n + ((which & 1) ? i1 : i)]);
  };
  const u64* pval = b.consts + sh.per_val;
  auto per = [&](uint32_t x) -> E2 { return gl::e2(pval[p3_per_offset(x) + (i & (((size_t)1 << p3_per_log_period(x)) - 1))]); };
  E2 num[AirProgram::MAX_AUX], den[AirProgram::MAX_AUX], pre[AirProgram::MAX_AUX];
  run_program<ExtF>(b.aux_prog, sh.n_aux_instr, b.consts, b.pub + (size_t)g * sh.n_public,
                    b.hdr + (size_t)g * sh.hdr_stride + sh.o_chal, load, per, [&](uint32_t out, const E2& x) {
                      if (out & 1) den[out >> 1] = x;
                      else num[out >> 1] = x;
                    });
  E2 acc = gl::e2(1);
  bool zero = false;
  for (uint32_t j = 0; j < AW; j++) {
    pre[j] = acc;
    if (gl::eq(den[j], gl::e2(0))) zero = true;
    else acc = gl::mul(acc, den[j]);
  }
  if (zero) set_p3_status(b.state + g, 1);
  E2 inv = zero ? gl::e2(0) : gl::inv(acc);
  u64* dst = b.tmp + (size_t)g * 2 * AW * n + i;
  for (uint32_t j = AW; j-- > 0;) {
    const E2 t = gl::mul(num[j], gl::mul(inv, pre[j]));   // zero for a failed row: inv is
    inv = gl::mul(inv, den[j]);
    dst[(size_t)(2 * j) * n] = t.a;
    dst[(size_t)(2 * j + 1) * n] = t.b;
  }
}

// The exclusive prefix sum in F_p^2 of every (proof, column) -- blockIdx.y = g AW + j, whose two component columns stand
// at tmp + blockIdx.y 2 n -- as k_zpp_scan_block / _totals / _finish do a running product: a block-local inclusive scan,
// an exclusive scan of the block totals, the add-back, in separate launches.  No block waits on another.
__global__ __launch_bounds__(P3_AUX_SCAN_BLOCK) void k_p3_aux_scan_block(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 sa[P3_AUX_SCAN_BLOCK], sb[P3_AUX_SCAN_BLOCK];
  const size_t n = (size_t)1 << sh.k, r = (size_t)blockIdx.x * P3_AUX_SCAN_BLOCK + threadIdx.x;
  const uint32_t t = threadIdx.x;
  u64* va = b.tmp + (size_t)blockIdx.y * 2 * n;
  u64* vb = va + n;
  E2 v = r < n ? E2{va[r], vb[r]} : gl::e2(0);
  sa[t] = v.a;
  sb[t] = v.b;
  __syncthreads();
  for (uint32_t off = 1; off < (uint32_t)P3_AUX_SCAN_BLOCK; off <<= 1) {
    const E2 o = t >= off ? E2{sa[t - off], sb[t - off]} : gl::e2(0);
    __syncthreads();
    v = gl::add(v, o);
    sa[t] = v.a;
    sb[t] = v.b;
    __syncthreads();
  }
  if (r < n) {
    va[r] = v.a;
    vb[r] = v.b;
  }
  if (t == P3_AUX_SCAN_BLOCK - 1) st_e2(b.atot + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2, v);
}
// the block totals of one (proof, column) per workgroup, tile after tile with a carry
__global__ __launch_bounds__(P3_AUX_TOTALS_TILE) void k_p3_aux_scan_totals(P3Bufs b, uint32_t n_blocks) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 sa[P3_AUX_TOTALS_TILE], sb[P3_AUX_TOTALS_TILE];
  __shared__ u64 carry_s[2];
  const uint32_t t = threadIdx.x;
  u64* bt = b.atot + (size_t)blockIdx.x * n_blocks * 2;
  if (t < 2) carry_s[t] = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n_blocks; base += P3_AUX_TOTALS_TILE) {
    const uint32_t i = base + t;
    E2 v = i < n_blocks ? ld_e2(bt + 2 * i) : gl::e2(0);
    sa[t] = v.a;
    sb[t] = v.b;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)P3_AUX_TOTALS_TILE; off <<= 1) {
      const E2 o = t >= off ? E2{sa[t - off], sb[t - off]} : gl::e2(0);
      __syncthreads();
      v = gl::add(v, o);
      sa[t] = v.a;
      sb[t] = v.b;
      __syncthreads();
    }
    const E2 carry = E2{carry_s[0], carry_s[1]};
    const E2 excl = t == 0 ? carry : gl::add(carry, E2{sa[t - 1], sb[t - 1]});
    __syncthreads();
    if (i < n_blocks) st_e2(bt + 2 * i, excl);
    if (t == P3_AUX_TOTALS_TILE - 1) st_e2(carry_s, gl::add(carry, v));
    __syncthreads();
  }
}
// S_j(r) = the totals of the blocks before r's + the inclusive sum up to r - 1 inside the block: to avals
__global__ __launch_bounds__(P3_AUX_SCAN_BLOCK) void k_p3_aux_scan_finish(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  const size_t n = (size_t)1 << sh.k, r = (size_t)blockIdx.x * P3_AUX_SCAN_BLOCK + threadIdx.x;
  if (r >= n) return;
  const u64* va = b.tmp + (size_t)blockIdx.y * 2 * n;
  E2 z = ld_e2(b.atot + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
  if (threadIdx.x > 0) z = gl::add(z, E2{va[r - 1], va[n + r - 1]});
  u64* out = b.avals + (size_t)blockIdx.y * 2 * n + r;
  out[0] = z.a;
  out[n] = z.b;
}

// One lane per point of the quotient coset 7 H_{n 2^lqd}.  Lane p takes the point stored at position p of the bit-reversed
// trace LDE (j = rev(p)), so the local row is read coalesced; its chunk is rev(p >> k) and its place in the chunk, in
// bit-reversed order, p mod n -- the order the inverse transform of the chunks takes.
// F = BaseF: an AIR without challenges and auxiliary columns.  F = ExtF: one with them, evaluated in F_p^2 throughout --
// every other operand embedded, an auxiliary column built from its two component columns of the proof's own LDE at the
// same two positions.
template <class F>
__global__ __launch_bounds__(256) void k_p3_quotient(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  const size_t n = (size_t)1 << sh.k, N2 = (size_t)1 << sh.L, nq = n << sh.lqd;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nq) return;
  const uint32_t g = blockIdx.y;
  const uint32_t j = gl::bitrev((u32)p, sh.k + sh.lqd);
  const u64 x = gl::mul(gl::GENERATOR, gl::pow(sh.w[sh.k + sh.lqd], j));
  const size_t i1 = (((size_t)j << (sh.B - sh.lqd)) + ((size_t)1 << sh.B)) & (N2 - 1);
  const size_t pos1 = gl::bitrev((u32)i1, sh.L);
  const u64* lde = b.tlde + (size_t)g * sh.W * N2;
  const uint32_t chunk = j & (sh.Q - 1);
  const u64 zhx = sh.zh[chunk];
  const u64 is_trans = gl::sub(x, sh.g_inv);
  const u64 sel[4] = {0, gl::mul(zhx, gl::inv(gl::sub(x, 1))), gl::mul(zhx, gl::inv(is_trans)), is_trans};
  const E2 alpha = ld_e2(b.state[g].alpha);
  // the preprocessed columns: the handle's shared LDE at the same two positions
  auto load = [&](int which, uint32_t c) -> u64 {
    return ((which & 2) ? b.plde : lde)[(size_t)c * N2 + ((which & 1) ? pos1 : p)];
  };
  // A periodic column at x_j: its table by j mod (P Q) -- the NATURAL index j, whose low bits are the reversed top bits of
  // p.  256 consecutive p share their top bits once n >= 256 P, so a block then reads one word: a plain load.
  const u64* ptab = b.consts + sh.per_tab;
  auto per = [&](uint32_t i) -> u64 {
    return ptab[((size_t)p3_per_offset(i) << sh.lqd) + (j & ((1u << (p3_per_log_period(i) + sh.lqd)) - 1))];
  };
  // every lane of the block reads the row of proof g: a plain load at a uniform address
  E2 acc;
  if constexpr (!F::EXT) {
    acc = run_air<BaseF>(b.prog, sh.n_instr, b.consts, b.pub + (size_t)g * sh.n_public, nullptr, load, per, sel, alpha);
  } else {
    const u64* alde = b.alde + (size_t)g * 2 * sh.AW * N2;
    auto eload = [&](int which, uint32_t c) -> E2 {
      if (!(which & 4)) return gl::e2(load(which, c));
      const u64* col = alde + (size_t)(2 * c) * N2 + ((which & 1) ? pos1 : p);
      return E2{col[0], col[N2]};
    };
    auto eper = [&](uint32_t i) -> E2 { return gl::e2(per(i)); };
    const E2 esel[4] = {gl::e2(0), gl::e2(sel[1]), gl::e2(sel[2]), gl::e2(sel[3])};
    acc = run_air<ExtF>(b.prog, sh.n_instr, b.consts, b.pub + (size_t)g * sh.n_public,
                        b.hdr + (size_t)g * sh.hdr_stride + sh.o_chal, eload, eper, esel, alpha);
  }
  const E2 q = gl::mul(acc, sh.zh_inv[chunk]);
  u64* dst = b.qv + (((size_t)chunk * sh.G + g) * 2) * n + (p & (n - 1));
  dst[0] = q.a;
  dst[n] = q.b;
}

// Openings: job < W: trace column at zeta; < 2 W: at zeta w_n; then the chunk components at zeta / s_c; then the shared
// preprocessed columns at this proof's zeta and zeta w_n, behind the chunk openings; then the 2 AW auxiliary base columns
// at the two points.  Lane t sums the
// coefficients t, t + 1024, ... by Horner in x^1024, scales by x^t; the block adds up.
__global__ __launch_bounds__(1024) void k_p3_eval(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  __shared__ u64 red[2 * 1024];
  const size_t n = (size_t)1 << sh.k;
  const uint32_t job = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  const u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  const u64* c;
  E2 x;
  uint32_t dst = 8 + 2 * job;   // the opening's place in the header
  if (job < 2 * sh.W) {
    c = b.tcoef + ((size_t)g * sh.W + (job % sh.W)) * n;
    x = ld_e2(hdr + sh.o_points + 2 * (job / sh.W));
  } else if (job >= 2 * sh.W + 2 * sh.Q + 2 * sh.PW) {   // the proof's auxiliary base columns, behind the auxiliary root
    const uint32_t aj = job - 2 * sh.W - 2 * sh.Q - 2 * sh.PW;
    c = b.acoef + ((size_t)g * 2 * sh.AW + (aj % (2 * sh.AW))) * n;
    x = ld_e2(hdr + sh.o_points + 2 * (aj / (2 * sh.AW)));
    dst += 4;
  } else if (job >= 2 * sh.W + 2 * sh.Q) {
    const uint32_t pj = job - 2 * sh.W - 2 * sh.Q;
    c = b.pcoef + (size_t)(pj % sh.PW) * n;
    x = ld_e2(hdr + sh.o_points + 2 * (pj / sh.PW));
  } else {
    const uint32_t q = job - 2 * sh.W;
    c = b.qcoef + (((size_t)(q >> 1) * sh.G + g) * 2 + (q & 1)) * n;
    x = ld_e2(hdr + sh.o_points + 4 + 2 * (q >> 1));
  }
  const E2 y = gl::pow(x, 1024);
  E2 acc = gl::e2(0);
  if (t < n) {
    size_t i = t + ((n - 1 - t) & ~(size_t)1023);
    for (;; i -= 1024) {
      acc = gl::mul(acc, y);
      acc.a = gl::add(acc.a, c[i]);
      if (i < 1024) break;
    }
    acc = gl::mul(acc, gl::pow(x, t));
  }
  red[2 * t] = acc.a;
  red[2 * t + 1] = acc.b;
  __syncthreads();
  for (uint32_t s = 512; s > 0; s >>= 1) {
    if (t < s) {
      red[2 * t] = gl::add(red[2 * t], red[2 * (t + s)]);
      red[2 * t + 1] = gl::add(red[2 * t + 1], red[2 * (t + s) + 1]);
    }
    __syncthreads();
  }
  if (t < 2) b.hdr[(size_t)g * sh.hdr_stride + dst + t] = red[t];
}

// The identity the verifier enforces (verifier.rs:169-239; p3_prover.cpp:306-329): a trace that violates the AIR fails here.
__global__ __launch_bounds__(64) void k_p3_identity(P3Shape sh, P3Bufs b) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= sh.G) return;
  const u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  const u64* open = hdr + 8;
  const E2 zeta = ld_e2(b.state[g].zeta), alpha = ld_e2(b.state[g].alpha);
  const E2 z_h = gl::sub(gl::exp_pow2(zeta, sh.k), gl::e2(1));
  const E2 is_trans = gl::sub(zeta, gl::e2(sh.g_inv));
  const E2 sel[4] = {gl::e2(0), gl::mul(z_h, gl::inv(gl::sub(zeta, gl::e2(1)))), gl::mul(z_h, gl::inv(is_trans)), is_trans};
  const u64* popen = open + 4 * sh.W + 4 * sh.Q;   // the preprocessed openings, behind the chunks'
  const u64* aopen = hdr + sh.o_aux + 4;           // the auxiliary openings, behind the auxiliary root
  auto load = [&](int which, uint32_t c) -> E2 {
    if (which & 4) {   // column c at the point: o[2 c] + X o[2 c + 1], as the chunks are recomposed
      const u64* o = aopen + 2 * (((which & 1) ? 2 * sh.AW : 0) + 2 * c);
      return gl::add(ld_e2(o), gl::mul(ld_e2(o + 2), E2{0, 1}));
    }
    return (which & 2) ? ld_e2(popen + 2 * (((which & 1) ? sh.PW : 0) + c)) : ld_e2(open + 2 * (((which & 1) ? sh.W : 0) + c));
  };
  const u64* pcoef = b.consts + sh.per_coef;
  auto per = [&](uint32_t i) -> E2 { return p3_periodic_at(pcoef + p3_per_offset(i), p3_per_log_period(i), sh.k, zeta); };
  const E2 acc = run_air<ExtF>(b.prog, sh.n_instr, b.consts, b.pub + (size_t)g * sh.n_public, hdr + sh.o_chal, load, per, sel, alpha);
  const E2 lhs = gl::mul(acc, gl::inv(z_h));
  E2 at_zeta[8];
  for (uint32_t j = 0; j < sh.Q; j++) at_zeta[j] = gl::sub(gl::exp_pow2(gl::mul(zeta, sh.s_inv[j]), sh.k), gl::e2(1));
  const u64* qz = open + 4 * sh.W;
  E2 rhs = gl::e2(0);
  for (uint32_t c = 0; c < sh.Q; c++) {
    E2 zp = gl::e2(1);
    for (uint32_t j = 0; j < sh.Q; j++) {
      if (j == c) continue;
      zp = gl::mul(zp, gl::mul(at_zeta[j], b.zfirst_inv[c * sh.Q + j]));
    }
    const E2 qa = ld_e2(qz + 4 * c), qb = ld_e2(qz + 4 * c + 2);
    rhs = gl::add(rhs, gl::mul(zp, gl::add(qa, gl::mul(qb, E2{0, 1}))));
  }
  if (!gl::eq(lhs, rhs)) set_p3_status(b.state + g, 1);
}

// FRI input (verifier.rs:296-338): one lane per LDE point, bit-reversed index.
__global__ __launch_bounds__(256) void k_p3_reduced(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  const size_t N2 = (size_t)1 << sh.L, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N2) return;
  const uint32_t g = blockIdx.y, W = sh.W, Q2 = 2 * sh.Q;
  const u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  const u64 *open = hdr + 8, *ap = hdr + sh.o_apow;
  const u64 x = gl::mul(gl::GENERATOR, gl::pow(sh.w[sh.L], gl::bitrev((u32)i, sh.L)));
  const E2 zeta = ld_e2(hdr + sh.o_points), zeta_next = ld_e2(hdr + sh.o_points + 2);
  const E2 inv_z = gl::inv(gl::sub(gl::e2(x), zeta)), inv_zn = gl::inv(gl::sub(gl::e2(x), zeta_next));
  const u64* tl = b.tlde + (size_t)g * W * N2 + i;
  E2 s_z = gl::e2(0), s_zn = gl::e2(0);
  for (uint32_t c = 0; c < W; c++) {
    const E2 v = gl::e2(tl[(size_t)c * N2]);
    s_z = gl::add(s_z, gl::mul(ld_e2(ap + 2 * c), gl::sub(v, ld_e2(open + 2 * c))));
    s_zn = gl::add(s_zn, gl::mul(ld_e2(ap + 2 * (W + c)), gl::sub(v, ld_e2(open + 2 * (W + c)))));
  }
  for (uint32_t c = 0; c < Q2; c++) {
    const E2 v = gl::e2(b.qlde[(((size_t)(c >> 1) * sh.G + g) * 2 + (c & 1)) * N2 + i]);
    s_z = gl::add(s_z, gl::mul(ld_e2(ap + 2 * (2 * W + c)), gl::sub(v, ld_e2(open + 2 * (2 * W + c)))));
  }
  // the third batch: the preprocessed matrix at zeta, then at zeta w_n; the powers go on behind the chunks'
  for (uint32_t c = 0; c < sh.PW; c++) {
    const E2 v = gl::e2(b.plde[(size_t)c * N2 + i]);
    const uint32_t t0 = 2 * W + Q2 + c, t1 = t0 + sh.PW;
    s_z = gl::add(s_z, gl::mul(ld_e2(ap + 2 * t0), gl::sub(v, ld_e2(open + 2 * t0))));
    s_zn = gl::add(s_zn, gl::mul(ld_e2(ap + 2 * t1), gl::sub(v, ld_e2(open + 2 * t1))));
  }
  // the last batch: the auxiliary matrix's 2 AW base columns at zeta, then at zeta w_n; their openings stand behind the
  // auxiliary root, four words further on than their powers
  for (uint32_t c = 0; c < 2 * sh.AW; c++) {
    const E2 v = gl::e2(b.alde[((size_t)g * 2 * sh.AW + c) * N2 + i]);
    const uint32_t t0 = 2 * W + Q2 + 2 * sh.PW + c, t1 = t0 + 2 * sh.AW;
    s_z = gl::add(s_z, gl::mul(ld_e2(ap + 2 * t0), gl::sub(v, ld_e2(open + 2 * t0 + 4))));
    s_zn = gl::add(s_zn, gl::mul(ld_e2(ap + 2 * t1), gl::sub(v, ld_e2(open + 2 * t1 + 4))));
  }
  st_e2(b.layers + (size_t)g * 4 * N2 + 2 * i, gl::add(gl::mul(s_z, inv_z), gl::mul(s_zn, inv_zn)));
}

// verifier.rs:441-516: evals[0] + (beta - x) (evals[1] - evals[0]) / (-x - x), x = w_m^rev(2 j);  1 / (-2 x) = -(1/2) x^-1
__device__ __forceinline__ E2 fold_pair(const P3Shape& sh, const u64* layer, size_t j, uint32_t lm, E2 beta) {
  const u32 br = gl::bitrev((u32)(2 * j), lm);
  const u64 x = gl::pow(sh.w[lm], br), x_inv = gl::pow(sh.w_inv[lm], br);
  const u64 den_inv = gl::neg(gl::mul(x_inv, (gl::P + 1) / 2));
  const E2 e0 = ld_e2(layer + 4 * j), e1 = ld_e2(layer + 4 * j + 2);
  const E2 num = gl::mul(gl::sub(e1, e0), gl::sub(beta, gl::e2(x)));
  return gl::add(e0, gl::mul(num, den_inv));
}
__global__ __launch_bounds__(256) void k_p3_fold(P3Shape sh, P3Bufs b, uint32_t round) {
  P25_WAVE_PRIO(P25_PRIO_BULK);
  const size_t N2 = (size_t)1 << sh.L, m = N2 >> round, j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m / 2) return;
  const uint32_t g = blockIdx.y;
  const E2 beta = ld_e2(b.hdr + (size_t)g * sh.hdr_stride + sh.o_betas + 2 * round);
  u64* base = b.layers + (size_t)g * 4 * N2;
  st_e2(base + p3_layer_off(N2, round + 1) + 2 * j, fold_pair(sh, base + p3_layer_off(N2, round), j, sh.L - round, beta));
}

// The FRI rounds from sh.tail_round on, one workgroup per proof: leaf hashes and tree levels with a 16-lane group per
// permutation, the challenger in the first wave, the fold by all lanes; then the check that what is left is constant.
__global__ __launch_bounds__(1024) void k_p3_fri_tail(P3Shape sh, P3Bufs b) {
  P25_WAVE_PRIO(P25_PRIO_CHAIN);
  __shared__ u64 rc[coop::P2_LDS_WORDS];
  coop::stage_poseidon2_rc(rc);
  const uint32_t g = blockIdx.x, tid = threadIdx.x, gid = tid >> 4, ngroups = 64;
  const int lane = tid & 63, rr = tid & 15;
  const size_t N2 = (size_t)1 << sh.L;
  P3State* s = b.state + g;
  u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  u64* layers = b.layers + (size_t)g * 4 * N2;
  u64* ftrees = b.ftrees + (size_t)g * 8 * N2;
  Chal ch;
  ch.lane = lane;
  ch.rc = rc;
  if (tid < 64) ch.load(s);
  for (uint32_t r = sh.tail_round; r < sh.k; r++) {
    const size_t m = N2 >> r, h = m / 2;
    u64* layer = layers + p3_layer_off(N2, r);
    u64* tree = ftrees + p3_ftree_off(N2, r);
    for (size_t i = gid; i < h; i += ngroups) {
      u64 v = rr < 4 ? layer[4 * i + rr] : 0;
      v = coop_p2(v, lane, rc);
      if (rr < 4) tree[4 * i + rr] = v;
    }
    __syncthreads();
    const uint32_t n_levels = sh.L - r - 1;
    for (uint32_t l = 0; l < n_levels; l++) {
      coop_level(tree + p3_level_off(h, l), tree + p3_level_off(h, l + 1), h >> (l + 1), gid, ngroups, lane, rc);
      __syncthreads();
    }
    if (tid < 64) {
      const u64* root = tree + p3_level_off(h, n_levels);
      u64* dst = hdr + sh.o_fri + 4 * r;
      if (lane < 4) dst[lane] = root[lane];
      ch.observe_digest(root);
      const E2 beta = ch.sample_ext();
      if (lane == 0) st_e2(hdr + sh.o_betas + 2 * r, beta);
    }
    __syncthreads();
    const E2 beta = ld_e2(hdr + sh.o_betas + 2 * r);
    u64* nxt = layers + p3_layer_off(N2, r + 1);
    for (size_t j = tid; j < h; j += 1024) st_e2(nxt + 2 * j, fold_pair(sh, layer, j, sh.L - r, beta));
    __syncthreads();
  }
  if (tid < 64) ch.store(s);
  if (tid == 0) {
    const u64* fin = layers + p3_layer_off(N2, sh.k);
    const E2 f0 = ld_e2(fin);
    bool constant = true;
    for (uint32_t i = 1; i < (1u << sh.B); i++) constant = constant && gl::eq(f0, ld_e2(fin + 2 * i));
    if (!constant) set_p3_status(s, 7);
    st_e2(s->final_poly, f0);
  }
}

// challenger.rs:159-168 for every candidate of the search window: the state with the pending inputs and the witness
// written over its first words, one permutation, the last word's low bits.  Lanes try their candidates in increasing order
// and leave once a smaller witness is known (k_pow_search), so the result is the smallest witness >= pow_start.
__global__ __launch_bounds__(256) void k_p3_pow_search(P3Shape sh, P3Bufs b, const u64* __restrict__ pow_starts, u64 total) {
  const uint32_t g = blockIdx.y;
  P3State* s = b.state + g;
  if (s->status != 0) return;
  const u64 start = pow_starts ? pow_starts[g] : 0;
  const u64 room = gl::P - 1 - start;   // candidates stay below p
  const u64 G = (u64)gridDim.x * blockDim.x, mask = ((u64)1 << sh.pow_bits) - 1;
  unsigned long long* result = reinterpret_cast<unsigned long long*>(&s->pow_witness);
  for (u64 off = (u64)blockIdx.x * blockDim.x + threadIdx.x; off < total && off <= room; off += G) {
    const u64 cand = start + off;
    if (__hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < cand) return;
    u64 v[12];
    const uint32_t pos = s->n_in;
#pragma unroll
    for (int i = 0; i < 12; i++) v[i] = (uint32_t)i < pos ? s->inb[i] : ((uint32_t)i == pos ? cand : s->st[i]);
    poseidon2::permute(v);
    // no `return` behind the atomic: see k_pow_search
    if ((v[11] & mask) == 0) atomicMin(result, (unsigned long long)cand);
  }
}

// Flattening (p3_prover.cpp:423-445).  Block q of a proof writes query q's two sections (the second ends in the third
// batch, row and path from the handle's shared LDE and tree, for an AIR with preprocessed columns), block 0 the fixed words and the
// public values behind the last query's section as well.  With auxiliary columns the header carries their root and openings
// and every query ends in their batch.  A failed proof's words are zeros, that tail included.
__global__ __launch_bounds__(64) void k_p3_gather(P3Shape sh, P3Bufs b, u64* __restrict__ out_base, size_t out_stride,
                                                  uint32_t* __restrict__ d_status) {
  const uint32_t qi = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  const size_t N2 = (size_t)1 << sh.L;
  const P3State* s = b.state + g;
  const u64* hdr = b.hdr + (size_t)g * sh.hdr_stride;
  u64* out = out_base + (size_t)g * out_stride;
  const uint32_t status = s->status;
  const uint32_t H = sh.hdr_words;
  u64* pa = out + H + (size_t)qi * sh.sz_a;
  const size_t mid = (size_t)H + (size_t)sh.num_queries * sh.sz_a;
  u64* pb = out + mid + 3 + (size_t)qi * sh.sz_b;
  u64* tail = out + mid + 3 + (size_t)sh.num_queries * sh.sz_b;
  if (qi == 0 && t == 0) d_status[g] = status;
  if (status != 0) {
    if (qi == 0) {
      for (uint32_t i = t; i < H; i += 64) out[i] = 0;
      if (t < 3) out[mid + t] = 0;
      for (uint32_t i = t; i < sh.n_public; i += 64) tail[i] = 0;
    }
    for (uint32_t i = t; i < sh.sz_a; i += 64) pa[i] = 0;
    for (uint32_t i = t; i < sh.sz_b; i += 64) pb[i] = 0;
    return;
  }
  if (qi == 0) {
    for (uint32_t i = t; i < H; i += 64) out[i] = hdr[i];
    if (t < 2) out[mid + t] = s->final_poly[t];
    if (t == 2) out[mid + 2] = s->pow_witness;
    for (uint32_t i = t; i < sh.n_public; i += 64) tail[i] = b.pub[(size_t)g * sh.n_public + i];
  }
  const uint32_t ix = reinterpret_cast<const uint32_t*>(hdr + sh.o_idx)[qi];
  {
    const u64* layers = b.layers + (size_t)g * 4 * N2;
    const u64* ftrees = b.ftrees + (size_t)g * 8 * N2;
    size_t idx = ix;
    u64* w = pa;
    for (uint32_t r = 0; r < sh.k; r++) {
      const size_t sib = idx ^ 1, pair = idx >> 1, h = N2 >> (r + 1);
      const uint32_t plen = sh.L - r - 1;
      if (t < 2) w[t] = layers[p3_layer_off(N2, r) + 2 * sib + t];
      const u64* tree = ftrees + p3_ftree_off(N2, r);
      for (uint32_t e = t; e < 4 * plen; e += 64) {
        const uint32_t l = e >> 2;
        w[2 + e] = tree[p3_level_off(h, l) + 4 * ((pair >> l) ^ 1) + (e & 3)];
      }
      w += 2 + 4 * plen;
      idx = pair;
    }
  }
  {
    u64* w = pb;
    for (uint32_t c = t; c < sh.W; c += 64) w[c] = b.tlde[((size_t)g * sh.W + c) * N2 + ix];
    w += sh.W;
    const u64* tt = b.ttree + (size_t)g * 8 * N2;
    for (uint32_t e = t; e < 4 * sh.L; e += 64) {
      const uint32_t l = e >> 2;
      w[e] = tt[p3_level_off(N2, l) + 4 * (((size_t)ix >> l) ^ 1) + (e & 3)];
    }
    w += 4 * sh.L;
    for (uint32_t c = t; c < 2 * sh.Q; c += 64) w[c] = b.qlde[(((size_t)(c >> 1) * sh.G + g) * 2 + (c & 1)) * N2 + ix];
    w += 2 * sh.Q;
    const u64* qt = b.qtree + (size_t)g * 8 * N2;
    for (uint32_t e = t; e < 4 * sh.L; e += 64) {
      const uint32_t l = e >> 2;
      w[e] = qt[p3_level_off(N2, l) + 4 * (((size_t)ix >> l) ^ 1) + (e & 3)];
    }
    if (sh.PW) {
      w += 4 * sh.L;
      for (uint32_t c = t; c < sh.PW; c += 64) w[c] = b.plde[(size_t)c * N2 + ix];
      w += sh.PW;
      for (uint32_t e = t; e < 4 * sh.L; e += 64) {
        const uint32_t l = e >> 2;
        w[e] = b.ptree[p3_level_off(N2, l) + 4 * (((size_t)ix >> l) ^ 1) + (e & 3)];
      }
    }
    if (sh.AW) {   // the last batch: row and path from the proof's own auxiliary LDE and tree
      w += 4 * sh.L;
      for (uint32_t c = t; c < 2 * sh.AW; c += 64) w[c] = b.alde[((size_t)g * 2 * sh.AW + c) * N2 + ix];
      w += 2 * sh.AW;
      const u64* at = b.atree + (size_t)g * 8 * N2;
      for (uint32_t e = t; e < 4 * sh.L; e += 64) {
        const uint32_t l = e >> 2;
        w[e] = at[p3_level_off(N2, l) + 4 * (((size_t)ix >> l) ^ 1) + (e & 3)];
      }
    }
  }
}

// levels of a tree whose leaf digests are in place: one lane per node while a level is large, 16 lanes per node below
// that, and the last levels of every proof in one workgroup
void build_tree(u64* tree, size_t tree_stride, size_t h, uint32_t G, hipStream_t st) {
  unsigned log_h = 0;
  while (((size_t)1 << log_h) < h) log_h++;
  unsigned l = 0;
  for (; l < log_h; l++) {
    const size_t nodes = h >> (l + 1);
    if (nodes * G <= (size_t)P3_TREE_COOP_MAX) break;
    hipLaunchKernelGGL(k_p3_tree_level, dim3((unsigned)((nodes + 255) / 256), G), dim3(256), 0, st, tree + p3_level_off(h, l),
                       tree + p3_level_off(h, l + 1), nodes, tree_stride);
  }
  for (; l < log_h; l++) {
    const size_t nodes = h >> (l + 1);
    if (nodes <= (size_t)P3_TREE_TOP_NODES) break;
    hipLaunchKernelGGL(k_p3_tree_coop, dim3((unsigned)((nodes + 15) / 16), G), dim3(256), 0, st, tree, tree_stride, h, l, 1u);
  }
  if (l < log_h) hipLaunchKernelGGL(k_p3_tree_coop, dim3(1, G), dim3(256), 0, st, tree, tree_stride, h, l, log_h - l);
}
}  // namespace

void p3_launch_transpose(const u64* d_traces, size_t trace_stride, const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  const size_t e = ((size_t)1 << s.k) * s.W;
  hipLaunchKernelGGL(k_p3_transpose, dim3((unsigned)((e + 255) / 256), s.G), dim3(256), 0, st, d_traces, trace_stride, b.tvals, s.W,
                     s.k);
}
void p3_launch_commit_cols(const u64* base, size_t proof_stride, size_t pair_stride, size_t col_stride, uint32_t width,
                           size_t h, u64* tree, size_t tree_stride, uint32_t G, hipStream_t st) {
  hipLaunchKernelGGL(k_p3_leaf_cols, dim3((unsigned)((h + 255) / 256), G), dim3(256), 0, st, base, proof_stride, pair_stride,
                     col_stride, width, h, tree, tree_stride);
  build_tree(tree, tree_stride, h, G, st);
}
void p3_launch_commit_rows4(const u64* rows, size_t rows_stride, size_t h, u64* tree, size_t tree_stride, uint32_t G,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_p3_leaf_rows4, dim3((unsigned)((h + 255) / 256), G), dim3(256), 0, st, rows, rows_stride, h, tree,
                     tree_stride);
  build_tree(tree, tree_stride, h, G, st);
}
void p3_launch_chain(const P3Shape& s, const P3Bufs& b, uint32_t phase, uint32_t round, hipStream_t st) {
  hipLaunchKernelGGL(k_p3_chain, dim3(1, s.G), dim3(64), 0, st, s, b, phase, round);
}
void p3_launch_aux_columns(const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  const size_t n = (size_t)1 << s.k;
  const unsigned blocks = (unsigned)((n + P3_AUX_SCAN_BLOCK - 1) / P3_AUX_SCAN_BLOCK);
  hipLaunchKernelGGL(k_p3_aux_terms, dim3((unsigned)((n + 255) / 256), s.G), dim3(256), 0, st, s, b);
  hipLaunchKernelGGL(k_p3_aux_scan_block, dim3(blocks, s.G * s.AW), dim3(P3_AUX_SCAN_BLOCK), 0, st, s, b);
  hipLaunchKernelGGL(k_p3_aux_scan_totals, dim3(s.G * s.AW), dim3(P3_AUX_TOTALS_TILE), 0, st, b, blocks);
  hipLaunchKernelGGL(k_p3_aux_scan_finish, dim3(blocks, s.G * s.AW), dim3(P3_AUX_SCAN_BLOCK), 0, st, s, b);
}
void p3_launch_quotient(const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  const size_t nq = (size_t)1 << (s.k + s.lqd);
  const dim3 grid((unsigned)((nq + 255) / 256), s.G);
  if (s.AW) hipLaunchKernelGGL(k_p3_quotient<ExtF>, grid, dim3(256), 0, st, s, b);
  else hipLaunchKernelGGL(k_p3_quotient<BaseF>, grid, dim3(256), 0, st, s, b);
}
void p3_launch_openings(const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  hipLaunchKernelGGL(k_p3_eval, dim3(2 * s.W + 2 * s.Q + 2 * s.PW + 4 * s.AW, s.G), dim3(1024), 0, st, s, b);
  hipLaunchKernelGGL(k_p3_identity, dim3((s.G + 63) / 64), dim3(64), 0, st, s, b);
}
void p3_launch_reduced(const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  const size_t N2 = (size_t)1 << s.L;
  hipLaunchKernelGGL(k_p3_reduced, dim3((unsigned)((N2 + 255) / 256), s.G), dim3(256), 0, st, s, b);
}
void p3_launch_fold(const P3Shape& s, const P3Bufs& b, uint32_t round, hipStream_t st) {
  const size_t half = ((size_t)1 << s.L) >> (round + 1);
  hipLaunchKernelGGL(k_p3_fold, dim3((unsigned)((half + 255) / 256), s.G), dim3(256), 0, st, s, b, round);
}
void p3_launch_fri_tail(const P3Shape& s, const P3Bufs& b, hipStream_t st) {
  hipLaunchKernelGGL(k_p3_fri_tail, dim3(s.G), dim3(1024), 0, st, s, b);
}
void p3_launch_pow_search(const P3Shape& s, const P3Bufs& b, const u64* d_pow_starts, hipStream_t st) {
  // the window of k_pow_search (kernels_transcript.hip): 2^(pow_bits + 6) candidates, at least 2^18; none of them a witness
  // has probability e^-64 and is reported as P25_ERR_INTERNAL by the launch that observes the witness
  const int wb = s.pow_bits < 12 ? 12 : (int)s.pow_bits;
  const int gb = wb < 16 ? wb : 16;
  hipLaunchKernelGGL(k_p3_pow_search, dim3(1u << (gb - 8), s.G), dim3(256), 0, st, s, b, d_pow_starts, (u64)1 << (wb + 6));
}
void p3_launch_gather(const P3Shape& s, const P3Bufs& b, u64* d_out, size_t out_stride, uint32_t* d_status, hipStream_t st) {
  hipLaunchKernelGGL(k_p3_gather, dim3(s.num_queries, s.G), dim3(64), 0, st, s, b, d_out, out_stride, d_status);
}

}  // namespace p25
