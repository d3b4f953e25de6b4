// Internal: the interpreter of an AIR's register program (P3AirDevice, p3_kernels.h), shared by the prover's quotient and
// identity kernels (kernels_p3.hip) and the verifier's identity lane (p3_verify_lanes.h).  Host and device: the verifier's
// lane functions also compile for the host.
#pragma once
#include "p3_kernels.h"

namespace p25 {

struct BaseF {
  typedef u64 T;
  static constexpr bool EXT = false;
  GL_HD static u64 cst(u64 v) { return v; }
  GL_HD static u64 add(u64 x, u64 y) { return gl::add(x, y); }
  GL_HD static u64 sub(u64 x, u64 y) { return gl::sub(x, y); }
  GL_HD static u64 mul(u64 x, u64 y) { return gl::mul(x, y); }
  // VerifierConstraintFolder::assert_zero: acc = acc * alpha + c
  GL_HD static gl::E2 fold(gl::E2 acc, gl::E2 alpha, u64 c) {
    acc = gl::mul(acc, alpha);
    acc.a = gl::add(acc.a, c);
    return acc;
  }
};
struct ExtF {
  typedef gl::E2 T;
  static constexpr bool EXT = true;   // the field an AIR with challenges or auxiliary columns is evaluated in
  GL_HD static gl::E2 cst(u64 v) { return gl::e2(v); }
  GL_HD static gl::E2 add(gl::E2 x, gl::E2 y) { return gl::add(x, y); }
  GL_HD static gl::E2 sub(gl::E2 x, gl::E2 y) { return gl::sub(x, y); }
  GL_HD static gl::E2 mul(gl::E2 x, gl::E2 y) { return gl::mul(x, y); }
  GL_HD static gl::E2 fold(gl::E2 acc, gl::E2 alpha, gl::E2 c) { return gl::add(gl::mul(acc, alpha), c); }
};
// A periodic column at zeta from its interpolant's P = 2^lp base-field coefficients: q(zeta^(n/P)), k - lp squarings and
// Horner (p3_prover.cpp's self-check; the identity lanes of the prover and the verifier, one lane per proof).
GL_HD gl::E2 p3_periodic_at(const u64* __restrict__ coef, uint32_t lp, uint32_t k, gl::E2 zeta) {
  const gl::E2 y = gl::exp_pow2(zeta, k - lp);
  gl::E2 acc = gl::e2(0);
  for (uint32_t i = 1u << lp; i-- > 0;) {
    acc = gl::mul(acc, y);
    acc.a = gl::add(acc.a, coef[i]);
  }
  return acc;
}
// Runs a register program: `load(which, column)` reads the row (which: P3_LOAD_*, the trace's, the preprocessed matrix's or,
// in ExtF alone, the auxiliary matrix's, current or next), `per(index)` gives the periodic column of a
// P3_OPND_PERIODIC operand (p3_per_log_period, p3_per_offset of its index) at the caller's point, `pub` is the proof's own
// row of public values (read only by P3_OPND_PUBLIC operands: may be null without them), `chal` the proof's challenges,
// two words each (read only by P3_OPND_CHALLENGE operands, which only an ExtF program has: may be null without them).
// Every P3_OP_EMIT hands its operand to emit(dst, value) in program order: a constraint and its `when` in the AIR's
// program, num_0, den_0, num_1, ... in the auxiliary columns' (P3AirDevice::aux_instr).
template <class F, class Load, class Per, class Emit>
GL_HD void run_program(const P3Instr* __restrict__ prog, uint32_t n_instr, const u64* __restrict__ consts,
                       const u64* __restrict__ pub, const u64* __restrict__ chal, Load load, Per per, Emit emit) {
  typedef typename F::T T;
  T slot[P3_MAX_LIVE];
  auto fetch = [&](uint32_t o) -> T {
    const uint32_t kind = o >> 28, i = o & 0x0fffffffu;
    if constexpr (F::EXT) {
      if (kind == P3_OPND_CHALLENGE) return gl::E2{chal[2 * i], chal[2 * i + 1]};
      if (kind == P3_OPND_AUX_LOCAL) return load(P3_LOAD_AUX_LOCAL, i);
      if (kind == P3_OPND_AUX_NEXT) return load(P3_LOAD_AUX_NEXT, i);
    }
    switch (kind) {
      case P3_OPND_SLOT: return slot[i];
      case P3_OPND_LOCAL: return load(P3_LOAD_LOCAL, i);
      case P3_OPND_NEXT: return load(P3_LOAD_NEXT, i);
      case P3_OPND_PREP_LOCAL: return load(P3_LOAD_PREP_LOCAL, i);
      case P3_OPND_PREP_NEXT: return load(P3_LOAD_PREP_NEXT, i);
      case P3_OPND_PUBLIC: return F::cst(pub[i]);
      case P3_OPND_PERIODIC: return per(i);
      default: return F::cst(consts[i]);
    }
  };
  for (uint32_t pc = 0; pc < n_instr; pc++) {
    const P3Instr in = prog[pc];
    const T x = fetch(in.a);
    if (in.op == P3_OP_EMIT) {
      emit(in.dst, x);
    } else {
      const T y = fetch(in.b);
      slot[in.dst] = in.op == P3_OP_ADD ? F::add(x, y) : in.op == P3_OP_SUB ? F::sub(x, y) : F::mul(x, y);
    }
  }
}
// The AIR's program: the constraints folded in program order.
template <class F, class Load, class Per>
GL_HD gl::E2 run_air(const P3Instr* __restrict__ prog, uint32_t n_instr, const u64* __restrict__ consts,
                     const u64* __restrict__ pub, const u64* __restrict__ chal, Load load, Per per, const typename F::T sel[4],
                     gl::E2 alpha) {
  gl::E2 acc = gl::e2(0);
  run_program<F>(prog, n_instr, consts, pub, chal, load, per, [&](uint32_t when, const typename F::T& x) {
    acc = F::fold(acc, alpha, when == 0 ? x : F::mul(sel[when & 3], x));
  });
  return acc;
}

}  // namespace p25
