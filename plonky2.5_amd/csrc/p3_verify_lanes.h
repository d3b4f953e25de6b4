// The plonky3 verifier's per-lane work, host and device: the verifier of src/p3/verifier.rs (the reference states it as a
// circuit) as plain functions of a batch description.  The kernels of kernels_p3_verify.hip only map lanes to (tree, proof,
// query) and merge the keys; everything here also compiles for the host (tests/native/p3_verify_lanes.cpp).
//   transcript_lane   challenger.rs:70-169 in the order of verifier.rs:135-139, 258, 363-382 (the proof's public values, if
//                     its AIR has any, observed behind the trace root), and the scan for words >= p;
//                     the device runs k_p3v_transcript (cooperative permutation) instead, this is its plain statement
//   identity_lane     verifier.rs:169-239: the quotient identity at zeta
//   fold_lane         verifier.rs:296-338 (reduced openings) and :419-518 (fold chain) of one query
//   merkle_lane       commit.rs:62-129 for one tree of one query: trace batch, quotient batch or a FRI round
//   verdict_lane      key -> P25_P3_REJECT_*
// A proof is the flat input vector of include/p25.h (`add_virtual_to` order, proof.rs:357-373, then its public values).
#pragma once
#include "p3_air_run.h"
#include "poseidon2.h"

namespace p25 {

// While a batch is being checked, a proof's status word holds the KEY of the earliest failed check found so far, in the
// statement order of verifier.rs (atomicMin: never the last writer); the verdict lane turns it into the code.
//   0                            a word >= p
//   1                            proof of work (:376)
//   2 + nb q + b                 input batch b (trace, quotient, preprocessed if any, auxiliary if any) of query q (:288-294;
//                                all queries before any FRI step); nb = 2 + (PW > 0) + (AW > 0)
//   F + q (k + 2)                a zero denominator in query q's reduced opening, F = 2 + nb num_queries: reported as the
//                                query's final-polynomial failure, ahead of its FRI rounds, whose leaves it spoils
//   F + q (k + 2) + 1 + r        FRI round r of query q (:471-481)
//   F + q (k + 2) + 1 + k        the final polynomial of query q (:413)
//   F + num_queries (k + 2)      the quotient identity (:239)
enum : uint32_t { P3VKEY_MALFORMED = 0, P3VKEY_POW = 1, P3VKEY_INPUT = 2, P3VKEY_NONE = 0xFFFFFFFFu };
enum : uint32_t {  // include/p25.h: P25_P3_REJECT_*
  P3V_REJECT_MALFORMED = 30, P3V_REJECT_POW = 31, P3V_REJECT_INPUT_MERKLE = 32, P3V_REJECT_FRI_MERKLE = 33,
  P3V_REJECT_FINAL_POLY = 34, P3V_REJECT_CONSTRAINTS = 35
};
// the per-proof challenge block (words); the query indices follow the betas, one word each, and for a handle with
// auxiliary columns its 2 NC challenge words follow those (c_chal)
enum : uint32_t { P3VC_ALPHA = 0, P3VC_ZETA = 2, P3VC_FRI_ALPHA = 4, P3VC_POW = 6, P3VC_BETAS = 8 };

struct P3VerifyArgs {
  const u64* proofs;   // proof p = num_inputs words at proofs + p * stride
  size_t stride;
  uint32_t n_proofs;
  u64* chal;           // scratch [n_proofs][chal_stride]
  u64* folded;         // scratch [n_proofs][num_queries][k][2]: the query's own value entering FRI round r
  uint32_t* status;    // [n_proofs]
  const P3Instr* prog;
  const u64* consts;
  const u64* zfirst_inv;   // [Q][Q]: 1 / Z_{D_j}(s_c)
  uint32_t k, B, L, Q, W, num_queries, pow_bits, n_instr, num_inputs;
  // word offsets in a proof: the opened values, the FRI roots, the queries' commit-phase openings (sz_a words each), the
  // final polynomial, the PoW witness, the queries' input openings (sz_b words each)
  uint32_t o_open, o_roots, o_qp, sz_a, o_final, o_pow, o_qo, sz_b;
  uint32_t c_idx, chal_stride;
  // the proof's public values: its last n_public words (num_inputs counts them), observed after the trace root and read
  // by the AIR's PUBLIC operands
  uint32_t n_public, o_public;
  // the periodic columns' coefficients: consts + per_coef (P3Shape::per_coef), read by the identity lane alone
  uint32_t per_coef;
  // the preprocessed columns: their count (0: none), the input batches of a query (2, or 3 with such columns) and the
  // handle's commitment, which the transcript observes behind the trace root and the third batch's paths must reach
  uint32_t PW, nb;
  const u64* prep_root;   // 4 words (the handle's: device memory on the device); unread when PW = 0
  // the auxiliary columns: NC challenges sampled behind the public values (to chal + c_chal), AW columns whose root --
  // the PROOF's words at o_aux -- is observed before alpha, whose openings follow it and whose batch is every query's last
  uint32_t NC, AW, o_aux, c_chal;
  u64 w_L, w_L_inv;    // primitive root of the LDE domain and its inverse
  u64 w_n, g_inv;      // generator of the trace domain and its inverse
  u64 neg2_inv;        // 1 / -2
  u64 s_inv[8];        // 1 / s_c, s_c the shift of chunk c's domain
};

GL_HD uint32_t p3v_key_fri(const P3VerifyArgs& a) { return P3VKEY_INPUT + a.nb * a.num_queries; }
GL_HD uint32_t p3v_key_constraints(const P3VerifyArgs& a) { return p3v_key_fri(a) + a.num_queries * (a.k + 2); }
// round r of a query's commit-phase openings: sibling_value (2 words), then L - r - 1 digests
GL_HD uint32_t p3v_round_off(const P3VerifyArgs& a, uint32_t r) { return 2 * r + 4 * (r * (a.L - 1) - r * (r - 1) / 2); }
// words of verifier scratch per proof
GL_HD size_t p3v_scratch_words(uint32_t k, uint32_t num_queries, uint32_t n_challenges = 0) {
  return 8 + 2 * (size_t)k + num_queries + 2 * (size_t)n_challenges + 2 * (size_t)num_queries * k;
}

namespace p3vlane {

using gl::E2;
GL_HD E2 ld(const u64* p) { return E2{p[0], p[1]}; }

// The sequential challenger (challenger.rs:70-169).
struct Challenger {
  u64 st[12], in[12], out[12];
  uint32_t n_in, n_out;
  GL_HD void init() {
    for (int i = 0; i < 12; i++) st[i] = in[i] = out[i] = 0;
    n_in = n_out = 0;
  }
  GL_HD void duplex() {
    for (uint32_t i = 0; i < n_in; i++) st[i] = in[i];
    n_in = 0;
    poseidon2::permute(st);
    for (int i = 0; i < 12; i++) out[i] = st[i];
    n_out = 12;
  }
  GL_HD void observe(u64 x) {
    n_out = 0;
    in[n_in++] = x;
    if (n_in == 12) duplex();
  }
  GL_HD u64 sample() {
    if (n_in > 0 || n_out == 0) duplex();
    return out[--n_out];
  }
};

// Proof p's challenge block; returns the key of the scan and the proof of work.
GL_HD uint32_t transcript_lane(const P3VerifyArgs& a, uint32_t p) {
  const u64* proof = a.proofs + (size_t)p * a.stride;
  u64* chal = a.chal + (size_t)p * a.chal_stride;
  bool bad = false;
  for (uint32_t i = 0; i < a.num_inputs; i++) bad = bad || proof[i] >= gl::P;
  Challenger ch;
  ch.init();
  auto draw = [&](uint32_t slot, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) chal[slot + i] = ch.sample();
  };
  for (int i = 0; i < 4; i++) ch.observe(proof[i]);
  if (a.PW)
    for (int i = 0; i < 4; i++) ch.observe(a.prep_root[i]);
  for (uint32_t i = 0; i < a.n_public; i++) ch.observe(proof[a.o_public + i]);
  if (a.AW) {
    draw(a.c_chal, 2 * a.NC);
    for (int i = 0; i < 4; i++) ch.observe(proof[a.o_aux + i]);
  }
  draw(P3VC_ALPHA, 2);
  for (int i = 0; i < 4; i++) ch.observe(proof[4 + i]);
  draw(P3VC_ZETA, 2);
  draw(P3VC_FRI_ALPHA, 2);
  for (uint32_t r = 0; r < a.k; r++) {
    for (int i = 0; i < 4; i++) ch.observe(proof[a.o_roots + 4 * r + i]);
    draw(P3VC_BETAS + 2 * r, 2);
  }
  ch.observe(proof[a.o_pow]);
  const u64 resp = ch.sample() & (((u64)1 << a.pow_bits) - 1);
  chal[P3VC_POW] = resp;
  chal[P3VC_POW + 1] = 0;
  for (uint32_t q = 0; q < a.num_queries; q++) chal[a.c_idx + q] = ch.sample() & (((u64)1 << a.L) - 1);
  return bad ? (uint32_t)P3VKEY_MALFORMED : resp != 0 ? (uint32_t)P3VKEY_POW : (uint32_t)P3VKEY_NONE;
}

// The quotient identity at zeta (verifier.rs:169-239): folded constraints * inv_zeroifier == sum_c zps_c * chunk_c(zeta).
GL_HD bool identity_lane(const P3VerifyArgs& a, uint32_t p) {
  const u64* proof = a.proofs + (size_t)p * a.stride;
  const u64* open = proof + a.o_open;
  const u64* chal = a.chal + (size_t)p * a.chal_stride;
  const E2 zeta = ld(chal + P3VC_ZETA), alpha = ld(chal + P3VC_ALPHA);
  // two_adic.rs:100-147: selectors at a point off the domain
  const E2 z_h = gl::sub(gl::exp_pow2(zeta, a.k), gl::e2(1));
  const E2 is_trans = gl::sub(zeta, gl::e2(a.g_inv));
  const E2 sel[4] = {gl::e2(0), gl::mul(z_h, gl::inv(gl::sub(zeta, gl::e2(1)))), gl::mul(z_h, gl::inv(is_trans)), is_trans};
  const uint32_t W = a.W;
  const u64* popen = open + 4 * W + 4 * a.Q;   // the preprocessed openings, behind the chunks'
  const u64* aopen = proof + a.o_aux + 4;      // the auxiliary openings, behind the auxiliary root
  auto load = [&](int which, uint32_t c) -> E2 {
    if (which & 4) {   // column c at the point: o[2 c] + X o[2 c + 1], as the chunks are recomposed
      const u64* o = aopen + 2 * (((which & 1) ? 2 * a.AW : 0) + 2 * c);
      return gl::add(ld(o), gl::mul(ld(o + 2), E2{0, 1}));
    }
    return (which & 2) ? ld(popen + 2 * (((which & 1) ? a.PW : 0) + c)) : ld(open + 2 * (((which & 1) ? W : 0) + c));
  };
  const u64* pcoef = a.consts + a.per_coef;
  auto per = [&](uint32_t i) -> E2 { return p3_periodic_at(pcoef + p3_per_offset(i), p3_per_log_period(i), a.k, zeta); };
  const E2 acc = run_air<ExtF>(a.prog, a.n_instr, a.consts, proof + a.o_public, chal + a.c_chal, load, per, sel, alpha);
  const E2 lhs = gl::mul(acc, gl::inv(z_h));
  // zps_c = prod_{j != c} Z_{D_j}(zeta) / Z_{D_j}(s_c),  Z_{D_j}(x) = (x / s_j)^n - 1
  E2 at_zeta[8];
  for (uint32_t j = 0; j < a.Q; j++) at_zeta[j] = gl::sub(gl::exp_pow2(gl::mul(zeta, a.s_inv[j]), a.k), gl::e2(1));
  const u64* qz = open + 4 * W;
  E2 rhs = gl::e2(0);
  for (uint32_t c = 0; c < a.Q; c++) {
    E2 zp = gl::e2(1);
    for (uint32_t j = 0; j < a.Q; j++)
      if (j != c) zp = gl::mul(zp, gl::mul(at_zeta[j], a.zfirst_inv[c * a.Q + j]));
    rhs = gl::add(rhs, gl::mul(zp, gl::add(ld(qz + 4 * c), gl::mul(ld(qz + 4 * c + 2), E2{0, 1}))));
  }
  return gl::eq(lhs, rhs);
}

// Query q of proof p: the reduced opening at the query's point, then the fold chain.  Leaves the query's own value of every
// round in a.folded (the round's Merkle leaf holds it) and returns the key of the final-polynomial comparison if it fails.
// A zero denominator x - z (zeta in the base field, on the LDE coset) counts as that failure, under a key ahead of the
// query's FRI rounds: the values it leaves for their leaves mean nothing.
GL_HD uint32_t fold_lane(const P3VerifyArgs& a, uint32_t p, uint32_t q) {
  const u64* proof = a.proofs + (size_t)p * a.stride;
  const u64* chal = a.chal + (size_t)p * a.chal_stride;
  u64* folded = a.folded + ((size_t)p * a.num_queries + q) * a.k * 2;
  const uint32_t W = a.W, L = a.L, Q2 = 2 * a.Q;
  uint32_t index = (uint32_t)chal[a.c_idx + q];
  const uint32_t rev = gl::bitrev(index, L);
  u64 x = gl::pow(a.w_L, rev), x_inv = gl::pow(a.w_L_inv, rev);
  const E2 zeta = ld(chal + P3VC_ZETA), fri_alpha = ld(chal + P3VC_FRI_ALPHA);
  // 1 / (x - zeta) and 1 / (x - zeta w_n) at x = 7 w_L^rev from one inversion
  const E2 cx = gl::e2(gl::mul(gl::GENERATOR, x));
  const E2 d0 = gl::sub(cx, zeta), d1 = gl::sub(cx, gl::mul(zeta, a.w_n));
  const E2 dd = gl::mul(d0, d1);
  const bool zero_den = gl::eq(dd, gl::e2(0));
  const E2 t = gl::inv(dd);
  const E2 inv_z = gl::mul(t, d1), inv_zn = gl::mul(t, d0);
  const u64* qo = proof + a.o_qo + (size_t)q * a.sz_b;
  const u64* row_t = qo;
  const u64* row_q = qo + W + 4 * L;
  const u64* open = proof + a.o_open;
  E2 ro = gl::e2(0), ap = gl::e2(1);
  for (uint32_t pt = 0; pt < 2; pt++)
    for (uint32_t c = 0; c < W; c++) {
      const E2 diff = gl::sub(gl::e2(row_t[c]), ld(open + 2 * (pt * W + c)));
      ro = gl::add(ro, gl::mul(ap, gl::mul(diff, pt ? inv_zn : inv_z)));
      ap = gl::mul(ap, fri_alpha);
    }
  for (uint32_t c = 0; c < Q2; c++) {   // the chunk matrices in order, two columns each, all opened at zeta
    const E2 diff = gl::sub(gl::e2(row_q[c]), ld(open + 4 * W + 2 * c));
    ro = gl::add(ro, gl::mul(ap, gl::mul(diff, inv_z)));
    ap = gl::mul(ap, fri_alpha);
  }
  if (a.PW) {   // the third batch: the preprocessed row at zeta, then at zeta w_n; the powers go on
    const u64* row_p = row_q + Q2 + 4 * L;
    const u64* popen = open + 4 * W + 2 * Q2;
    for (uint32_t pt = 0; pt < 2; pt++)
      for (uint32_t c = 0; c < a.PW; c++) {
        const E2 diff = gl::sub(gl::e2(row_p[c]), ld(popen + 2 * (pt * a.PW + c)));
        ro = gl::add(ro, gl::mul(ap, gl::mul(diff, pt ? inv_zn : inv_z)));
        ap = gl::mul(ap, fri_alpha);
      }
  }
  if (a.AW) {   // the last batch: the auxiliary row's 2 AW words at zeta, then at zeta w_n; the powers go on
    const u64* row_a = qo + a.sz_b - 4 * L - 2 * a.AW;
    const u64* aopen = proof + a.o_aux + 4;
    for (uint32_t pt = 0; pt < 2; pt++)
      for (uint32_t c = 0; c < 2 * a.AW; c++) {
        const E2 diff = gl::sub(gl::e2(row_a[c]), ld(aopen + 2 * (pt * 2 * a.AW + c)));
        ro = gl::add(ro, gl::mul(ap, gl::mul(diff, pt ? inv_zn : inv_z)));
        ap = gl::mul(ap, fri_alpha);
      }
  }
  // every matrix has the height of the LDE domain: the reduced opening enters before round 0 and nothing later
  E2 f = ro;
  const u64* qp = proof + a.o_qp + (size_t)q * a.sz_a;
  for (uint32_t r = 0; r < a.k; r++) {
    folded[2 * r] = f.a;
    folded[2 * r + 1] = f.b;
    const E2 sib = ld(qp + p3v_round_off(a, r));
    const E2 beta = ld(chal + P3VC_BETAS + 2 * r);
    const bool odd = index & 1;
    const E2 e0 = odd ? sib : f, e1 = odd ? f : sib;
    // evals[0] + (beta - xs[0]) (evals[1] - evals[0]) / (xs[1] - xs[0]),  xs = (x, -x) for an even index, (-x, x) for an odd one
    const u64 xs0 = odd ? gl::neg(x) : x;
    const u64 den_inv = gl::mul(a.neg2_inv, odd ? gl::neg(x_inv) : x_inv);
    const E2 num = gl::mul(gl::sub(e1, e0), gl::sub(beta, gl::e2(xs0)));
    f = gl::add(e0, gl::mul(num, den_inv));
    index >>= 1;
    x = gl::mul(x, x);
    x_inv = gl::mul(x_inv, x_inv);
  }
  const uint32_t key0 = p3v_key_fri(a) + q * (a.k + 2);
  if (zero_den) return key0;
  return gl::eq(f, ld(proof + a.o_final)) ? (uint32_t)P3VKEY_NONE : key0 + 1 + a.k;
}

// Tree `tree` of query q of proof p: 0 the trace batch, 1 the quotient batch (all chunk matrices have one height: their rows
// are hashed as one), with preprocessed columns 2 their batch, checked against the handle's root, with auxiliary columns
// a.nb - 1 theirs, checked against the proof's aux_commit; a.nb + r the
// commit of FRI round r, whose leaf is the pair (own value, sibling value) in index order.
// hash_iter_slices (commit.rs:23-46) of the leaf, then a compress per sibling; leaf chunks and path steps share ONE
// permutation call site.
GL_HD uint32_t merkle_lane(const P3VerifyArgs& a, uint32_t tree, uint32_t p, uint32_t q) {
  const u64* proof = a.proofs + (size_t)p * a.stride;
  uint32_t idx = (uint32_t)a.chal[(size_t)p * a.chal_stride + a.c_idx + q];
  const u64* qo = proof + a.o_qo + (size_t)q * a.sz_b;
  const u64 *leaf, *sibs, *root;
  uint32_t width, depth, key;
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = 0;
  const bool prep = a.PW && tree == 2;
  const bool aux = a.AW && tree == a.nb - 1;   // the last batch
  if (tree < a.nb) {
    width = aux ? 2 * a.AW : prep ? a.PW : tree ? 2 * a.Q : a.W;
    leaf = aux ? qo + a.sz_b - 4 * a.L - 2 * a.AW : qo + (tree ? a.W + 4 * a.L : 0) + (prep ? 2 * a.Q + 4 * a.L : 0);
    sibs = leaf + width;
    depth = a.L;
    // the preprocessed batch's root is the handle's, not the proof's; the auxiliary batch's is the proof's own aux_commit
    root = aux ? proof + a.o_aux : prep ? a.prep_root : proof + 4 * tree;
    key = P3VKEY_INPUT + a.nb * q + tree;
  } else {
    const uint32_t r = tree - a.nb;
    const u64* step = proof + a.o_qp + (size_t)q * a.sz_a + p3v_round_off(a, r);
    const u64* own = a.folded + (((size_t)p * a.num_queries + q) * a.k + r) * 2;
    idx >>= r;
    const bool odd = idx & 1;
    idx >>= 1;
    s[0] = odd ? step[0] : own[0];
    s[1] = odd ? step[1] : own[1];
    s[2] = odd ? own[0] : step[0];
    s[3] = odd ? own[1] : step[1];
    width = 4;
    leaf = nullptr;
    sibs = step + 2;
    depth = a.L - r - 1;
    root = proof + a.o_roots + 4 * r;
    key = p3v_key_fri(a) + q * (a.k + 2) + 1 + r;
  }
  const uint32_t n_chunks = (width + 3) / 4;
  for (uint32_t it = 0; it < n_chunks + depth; it++) {
    if (it < n_chunks) {
      if (leaf) {
        const uint32_t m = width - 4 * it;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if ((uint32_t)i < m) s[i] = leaf[4 * it + i];
      }
    } else {
      const u64* sib = sibs + 4 * (it - n_chunks);
      const bool right = idx & 1;
      idx >>= 1;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u64 d = s[i], o = sib[i];
        s[i] = right ? o : d;
        s[4 + i] = right ? d : o;
        s[8 + i] = 0;
      }
    }
    poseidon2::permute(s);
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; i++) ok = ok && s[i] == root[i];
  return ok ? (uint32_t)P3VKEY_NONE : key;
}

GL_HD uint32_t verdict_lane(const P3VerifyArgs& a, uint32_t key) {
  if (key == P3VKEY_NONE) return 0;
  if (key == P3VKEY_MALFORMED) return P3V_REJECT_MALFORMED;
  if (key == P3VKEY_POW) return P3V_REJECT_POW;
  if (key < p3v_key_fri(a)) return P3V_REJECT_INPUT_MERKLE;
  if (key >= p3v_key_constraints(a)) return P3V_REJECT_CONSTRAINTS;
  const uint32_t step = (key - p3v_key_fri(a)) % (a.k + 2);
  return step == 0 || step == a.k + 1 ? P3V_REJECT_FINAL_POLY : P3V_REJECT_FRI_MERKLE;
}

}  // namespace p3vlane

// the five stages of a batch, one launch each, on `st` (kernels_p3_verify.hip)
void launch_p3_verify(const P3VerifyArgs& a, hipStream_t st);

}  // namespace p25
