// The verifier's per-lane work, host and device: what one lane of k_verify_vanishing / k_verify_fri / k_verify_verdict
// (kernels_verify.hip) computes, as plain functions of the batch description.  The kernels only map lanes to (task,
// proof, query) and merge the keys; everything here also compiles for the host, where it runs under the sanitizers.
#pragma once
#include "ext_gates.h"
#include "verify_kernels.h"

namespace p25 {
namespace vlane {

using extf::ext;
typedef extf::Ext E;   // (p25::Ext is the builder's pair of targets)

struct OpenedWires {  // wire i of the opened row: an extension element of the proof's `wires` openings
  const u64* p;
  GL_HD E operator()(int i) const { return E{p[2 * i], p[2 * i + 1]}; }
};
GL_HD E load_ext(const u64* p, uint32_t i) { return E{p[2 * i], p[2 * i + 1]}; }

// Task `task` of proof p: gate type `task` (< n_gates), or the L_0 term and the permutation argument of challenge
// task - n_gates.  Leaves the task's share of the two alpha folds in a.partial.
GL_HD void vanishing_lane(const VerifyArgs& a, uint32_t task, uint32_t p) {
  const uint32_t n_tasks = a.n_gates + 2;
  const u64* proof = a.proofs + (size_t)p * a.stride;
  const u64* chal = a.chal + (size_t)p * VCH_WORDS;
  const uint32_t NP = a.num_partial_products;
  const E one = ext(1);
  // term order (vanishing_poly.rs): 2 L_0 terms | 2 x (NP + 1) partial-product terms | the gate constraints
  extf::AlphaFold fold;
  fold.start(chal[CH_ALPHAS], chal[CH_ALPHAS + 1]);
  if (task < a.n_gates) {
    const GateEntry g = a.gates[task];
    const E s = load_ext(proof + a.constants, g.selector_index);
    E filter = one;
    for (uint32_t k = g.group_start; k < g.group_end; k++)
      if (k != task) filter = filter * (ext(k) - s);
    if (a.num_selectors > 1) filter = filter * (ext(0xFFFFFFFFull) - s);   // UNUSED_SELECTOR
    fold.filter = filter;
    fold.seek(2 * (2 + NP));
    E pih[4];
    for (int i = 0; i < 4; i++) pih[i] = ext(chal[VCH_PI_HASH + i]);
    const OpenedWires w{proof + a.wires};
    extf::eval_gate(g.kind, w, load_ext(proof + a.constants, a.num_selectors), load_ext(proof + a.constants, a.num_selectors + 1),
                    pih, fold);
  } else {
    const uint32_t i = task - a.n_gates;
    const E zeta{chal[CH_ZETA], chal[CH_ZETA + 1]};
    const E z_h = extf::exp_pow2(zeta, a.degree_bits) - one;
    const E l0 = z_h * extf::inv((zeta - one) * ((u64)1 << a.degree_bits));
    const E z = load_ext(proof + a.zs, i);
    fold.seek(i);
    fold(l0 * (z - one));
    fold.seek(2 + i * (NP + 1));
    const u64 beta = chal[CH_BETAS + i];
    const E gamma = ext(chal[CH_GAMMAS + i]);
    const uint32_t Q = a.quotient_degree_factor, RW = a.num_routed;
    for (uint32_t ch = 0; ch * Q < RW; ch++) {
      const E prev = ch == 0 ? z : load_ext(proof + a.pps, i * NP + ch - 1);
      const E next = ch == NP ? load_ext(proof + a.zs_next, i) : load_ext(proof + a.pps, i * NP + ch);
      E num = one, den = one;
      for (uint32_t j = ch * Q; j < (ch + 1) * Q && j < RW; j++) {
        const E wj = load_ext(proof + a.wires, j);
        num = num * (wj + zeta * gl::mul(a.k_is[j], beta) + gamma);
        den = den * (wj + load_ext(proof + a.sigmas, j) * beta + gamma);
      }
      fold(prev * num - next * den);
    }
  }
  u64* out = a.partial + ((size_t)p * n_tasks + task) * 4;
  out[0] = fold.acc[0].a;
  out[1] = fold.acc[0].b;
  out[2] = fold.acc[1].a;
  out[3] = fold.acc[1].b;
}

// One Merkle path (upstream merkle_proofs.rs `verify_merkle_proof_to_cap`): hash_or_noop of the leaf, then a
// two_to_one per sibling.  Leaf chunks and path steps share ONE permutation call site, so a wave whose lanes sit at
// different steps does not serialise two copies of the permutation.
GL_HD bool merkle_path_ok(const u64* leaf, uint32_t width, uint32_t depth, uint32_t idx, const u64* cap) {
  const u64* sibs = leaf + width;
  const uint32_t n_chunks = width > 4 ? (width + 7) / 8 : 0;
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = 0;
  if (!n_chunks) {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if ((uint32_t)i < width) s[i] = leaf[i];
  }
  for (uint32_t it = 0; it < n_chunks + depth; it++) {
    if (it < n_chunks) {
      const uint32_t m = width - 8 * it;
#pragma unroll
      for (int i = 0; i < 8; i++)
        if ((uint32_t)i < m) s[i] = leaf[8 * it + i];
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
    poseidon::permute(s);
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; i++) ok = ok && s[i] == cap[4 * idx + i];
  return ok;
}

// Task `task` of query q of proof p: the Merkle path of tree `task` (< 4 + n_layers), or the query's arithmetic.
// Returns the key of the check that failed (the first one, for the arithmetic), VKEY_NONE if none did.
GL_HD uint32_t fri_lane(const VerifyArgs& a, uint32_t task, uint32_t p, uint32_t q) {
  const uint32_t n_trees = 4 + a.n_layers;
  const u64* proof = a.proofs + (size_t)p * a.stride;
  const u64* chal = a.chal + (size_t)p * VCH_WORDS;
  const u64* round = proof + a.queries + (size_t)q * a.query_stride;
  const uint32_t lde_bits = a.degree_bits + a.rate_bits;
  const uint32_t x_index = (uint32_t)(chal[CH_QUERIES + q] & (((u64)1 << lde_bits) - 1));
  const uint32_t key0 = VKEY_QUERY + q * VKEY_QUERY_STEPS;

  if (task < n_trees) {
    const u64* cap = task == 0 ? a.cs_cap : proof + a.tree_cap[task];
    if (!merkle_path_ok(round + a.tree_off[task], a.tree_width[task], a.tree_depth[task], x_index >> a.tree_shift[task], cap))
      return key0 + (task < 4 ? task : 5 + 2 * (task - 4));
    return VKEY_NONE;
  }

  // the query's arithmetic (fri/verifier.rs `fri_combine_initial`, `fri_verifier_query_round`)
  const E zeta{chal[CH_ZETA], chal[CH_ZETA + 1]}, alpha{chal[CH_FRI_ALPHA], chal[CH_FRI_ALPHA + 1]};
  const E zeta_next = zeta * a.g_n;
  // sum_i alpha^i v_i over the extension elements at words [lo, hi) of the proof, on top of `acc` for the elements behind
  auto reduce_openings = [&](E acc, uint32_t lo, uint32_t hi) {
    for (uint32_t i = hi; i > lo; i -= 2) acc = acc * alpha + E{proof[i - 2], proof[i - 1]};
    return acc;
  };
  const E red0 = reduce_openings(reduce_openings(ext(0), a.pps, a.fri_caps), a.constants, a.zs_next);
  const E red1 = reduce_openings(ext(0), a.zs_next, a.pps);
  E e0 = ext(0), e1 = ext(0);
  for (int t = 3; t >= 0; t--) {
    const u64* leaf = round + a.tree_off[t];
    for (uint32_t i = a.tree_width[t]; i > 0; i--) {
      e0 = e0 * alpha;
      e0.a = gl::add(e0.a, leaf[i - 1]);
    }
  }
  for (int k = 1; k >= 0; k--) {   // the batch opened at g zeta: the Z polynomials, the first columns of oracle 2
    e1 = e1 * alpha;
    e1.a = gl::add(e1.a, round[a.tree_off[2] + k]);
  }
  const u64 sx = gl::mul(gl::GENERATOR, gl::pow(a.w_lde, gl::bitrev(x_index, lde_bits)));
  E sum = (e0 - red0) * extf::inv(ext(sx) - zeta);
  sum = sum * (alpha * alpha) + (e1 - red1) * extf::inv(ext(sx) - zeta_next);
  E old_eval = sum * sx;   // the batch polynomial is multiplied by X (upstream PR #436)

  u64 subgroup_x = sx;
  uint32_t index = x_index;
  for (uint32_t l = 0; l < a.n_layers; l++) {
    const uint32_t ab = a.arity_bits[l], arity = 1u << ab;
    const u64* evals = round + a.tree_off[4 + l];
    const uint32_t within = index & (arity - 1);
    if (load_ext(evals, within) != old_eval) return key0 + 4 + 2 * l;
    // interpolate the coset's values at beta (`compute_evaluation`): point i = coset_start * g^i holds evals[rev(i)]
    const E beta{chal[CH_FRI_BETAS + 2 * l], chal[CH_FRI_BETAS + 2 * l + 1]};
    const u64 ga = gl::root_of_unity(ab);
    u64 xs[1 << VERIFY_MAX_ARITY_BITS];
    u64 y = gl::mul(subgroup_x, gl::pow(ga, arity - gl::bitrev(within, ab)));
    for (uint32_t i = 0; i < arity; i++) {
      xs[i] = y;
      y = gl::mul(y, ga);
    }
    E acc = ext(0);
    for (uint32_t i = 0; i < arity; i++) {
      E numer = ext(1);
      u64 denom = 1;
      for (uint32_t j = 0; j < arity; j++)
        if (j != i) {
          numer = numer * (beta - ext(xs[j]));
          denom = gl::mul(denom, gl::sub(xs[i], xs[j]));
        }
      acc = acc + load_ext(evals, gl::bitrev(i, ab)) * (numer * gl::inv(denom));
    }
    old_eval = acc;
    subgroup_x = gl::exp_pow2(subgroup_x, ab);
    index >>= ab;
  }
  E fin = ext(0);
  for (uint32_t k = a.final_poly_len; k > 0; k--) fin = fin * subgroup_x + load_ext(proof + a.final_poly, k - 1);
  return fin != old_eval ? key0 + 4 + 2 * a.n_layers : (uint32_t)VKEY_NONE;
}

GL_HD uint32_t leading_zeros(u64 x) { return x ? (uint32_t)__builtin_clzll(x) : 64u; }

// Proof p's verdict from the key the earlier stages left: the vanishing identity and the PoW are checked here.
GL_HD uint32_t verdict_lane(const VerifyArgs& a, uint32_t p, uint32_t key) {
  const u64* proof = a.proofs + (size_t)p * a.stride;
  const u64* chal = a.chal + (size_t)p * VCH_WORDS;
  if (key > VKEY_VANISHING) {
    // vanishing(zeta) == Z_H(zeta) * sum_k zeta^(n k) t_k(zeta), for both alphas
    const uint32_t n_tasks = a.n_gates + 2, Q = a.quotient_degree_factor;
    const u64* part = a.partial + (size_t)p * n_tasks * 4;
    E van[2] = {ext(0), ext(0)};
    for (uint32_t t = 0; t < n_tasks; t++)
      for (int i = 0; i < 2; i++) van[i] = van[i] + E{part[4 * t + 2 * i], part[4 * t + 2 * i + 1]};
    const E zeta_n = extf::exp_pow2(E{chal[CH_ZETA], chal[CH_ZETA + 1]}, a.degree_bits);
    const E z_h = zeta_n - ext(1);
    bool ok = true;
    for (uint32_t i = 0; i < 2; i++) {
      E t = ext(0);
      for (uint32_t k = Q; k > 0; k--) t = t * zeta_n + load_ext(proof + a.quotient, i * Q + k - 1);
      ok = ok && van[i] == z_h * t;
    }
    if (!ok)
      key = VKEY_VANISHING;
    else if (leading_zeros(chal[CH_POW_RESPONSE]) < a.pow_bits && key > VKEY_POW)
      key = VKEY_POW;
  }
  uint32_t code = 0;
  if (key == VKEY_MALFORMED) code = V_REJECT_MALFORMED;
  else if (key == VKEY_VANISHING) code = V_REJECT_VANISHING;
  else if (key == VKEY_POW) code = V_REJECT_POW;
  else if (key != VKEY_NONE) {
    const uint32_t step = (key - VKEY_QUERY) % VKEY_QUERY_STEPS;
    code = step < 4 ? V_REJECT_INITIAL_MERKLE
                    : (step == 4 + 2 * a.n_layers ? V_REJECT_FINAL_POLY : ((step & 1) ? V_REJECT_FRI_MERKLE : V_REJECT_FRI_EVAL));
  }
  return code;
}

}  // namespace vlane
}  // namespace p25
