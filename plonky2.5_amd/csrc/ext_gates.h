// Gate constraints over the quadratic extension F_p[X]/(X^2 - 7): what the VERIFIER evaluates at the opening
// point zeta (upstream plonky2 @ 3de92d9 vanishing_poly.rs `eval_vanishing_poly` with every gate's
// `eval_unfiltered`; the reference's own gates: poseidon2_gate.rs:150-231, arithmetic_u32.rs:106-165,
// interleave_u32.rs:102-142, uninterleave_to_u32.rs:114-163).
//
// The prover's evaluators (kernels_quotient.hip) are base-field, lazy and tied to the LDE columns of one row; here a
// "wire" is an opened value in F_p^2, there is one row per proof, and everything is canonical arithmetic on an `Ext`
// value type.  Constraints are handed to a sink in the gate's constraint order; the sink does the selector filter and
// the fold with the powers of alpha (AlphaFold below).  Loops are kept as loops: this code runs once per proof.
#pragma once
#include "builder.h"
#include "poseidon.h"
#include "poseidon2.h"

namespace p25 {
namespace extf {

struct Ext {
  u64 a, b;  // a + b X, both canonical
};
GL_HD Ext ext(u64 a, u64 b = 0) { return Ext{a, b}; }
GL_HD Ext operator+(Ext x, Ext y) { return Ext{gl::add(x.a, y.a), gl::add(x.b, y.b)}; }
GL_HD Ext operator-(Ext x, Ext y) { return Ext{gl::sub(x.a, y.a), gl::sub(x.b, y.b)}; }
GL_HD Ext operator*(Ext x, Ext y) {
  return Ext{gl::add(gl::mul(x.a, y.a), gl::mul(gl::EXT_W, gl::mul(x.b, y.b))), gl::add(gl::mul(x.a, y.b), gl::mul(x.b, y.a))};
}
GL_HD Ext operator*(Ext x, u64 s) { return Ext{gl::mul(x.a, s), gl::mul(x.b, s)}; }
GL_HD bool operator==(Ext x, Ext y) { return x.a == y.a && x.b == y.b; }
GL_HD bool operator!=(Ext x, Ext y) { return !(x == y); }
GL_HD Ext inv(Ext x) {  // inv(0) = 0
  const u64 ni = gl::inv(gl::sub(gl::mul(x.a, x.a), gl::mul(gl::EXT_W, gl::mul(x.b, x.b))));
  return Ext{gl::mul(x.a, ni), gl::mul(gl::neg(x.b), ni)};
}
GL_HD Ext exp_pow2(Ext x, unsigned k) {
  for (unsigned i = 0; i < k; i++) x = x * x;
  return x;
}
GL_HD Ext pow(Ext x, u64 e) {
  Ext r = ext(1);
  for (; e; e >>= 1) {
    if (e & 1) r = r * x;
    x = x * x;
  }
  return r;
}
GL_HD Ext pow7(Ext x) {
  const Ext x2 = x * x, x3 = x2 * x;
  return x3 * (x2 * x2);
}
// an element of the algebra F[X]/(X^2 - 7) whose two coordinates are wires, i.e. themselves in F_p^2
struct Alg {
  Ext a, b;
};
GL_HD Alg alg_mul(Alg x, Alg y) { return Alg{x.a * y.a + (x.b * y.b) * gl::EXT_W, x.a * y.b + x.b * y.a}; }

// Sink of a proof's vanishing terms: term number t enters accumulator i as filter * term * alpha_i^t, for both alphas.
struct AlphaFold {
  u64 alpha[2], pw[2];
  Ext acc[2], filter;
  GL_HD void start(u64 a0, u64 a1) {
    alpha[0] = a0;
    alpha[1] = a1;
    acc[0] = acc[1] = ext(0);
    filter = ext(1);
    seek(0);
  }
  GL_HD void seek(uint32_t t) {
    pw[0] = gl::pow(alpha[0], t);
    pw[1] = gl::pow(alpha[1], t);
  }
  GL_HD void operator()(Ext c) {
    const Ext f = filter * c;
    for (int i = 0; i < 2; i++) {
      acc[i] = acc[i] + f * pw[i];
      pw[i] = gl::mul(pw[i], alpha[i]);
    }
  }
};

// ---- linear layers of the two permutations on extension-valued states --------------------------------------------
GL_HD void poseidon_mds(Ext s[12]) {  // circ(MDS_CIRC) + diag(8, 0, ..., 0)
  Ext o[12];
  for (int r = 0; r < 12; r++) {
    Ext t = r == 0 ? s[0] * (u64)poseidon::MDS_DIAG0 : ext(0);
    for (int i = 0; i < 12; i++) t = t + s[(i + r) % 12] * (u64)poseidon::MDS_CIRC[i];
    o[r] = t;
  }
  for (int r = 0; r < 12; r++) s[r] = o[r];
}
GL_HD void p2_external(Ext s[12]) {  // poseidon2.rs:126-147, 184-213
  for (int blk = 0; blk < 3; blk++) {
    Ext* x = s + 4 * blk;
    const Ext t0 = x[0] + x[1], t1 = x[2] + x[3];
    const Ext t2 = t1 + x[1] * (u64)2, t3 = t0 + x[3] * (u64)2;
    const Ext t4 = t3 + t1 * (u64)4, t5 = t2 + t0 * (u64)4;
    x[0] = t3 + t5;
    x[1] = t5;
    x[2] = t2 + t4;
    x[3] = t4;
  }
  Ext col[4];
  for (int l = 0; l < 4; l++) col[l] = s[l] + s[4 + l] + s[8 + l];
  for (int i = 0; i < 12; i++) s[i] = s[i] + col[i & 3];
}
GL_HD void p2_internal(Ext s[12]) {  // poseidon2.rs:163-182
  Ext sum = s[0];
  for (int i = 1; i < 12; i++) sum = sum + s[i];
  for (int i = 0; i < 12; i++) s[i] = s[i] * (poseidon2::P2_MAT_DIAG_M_1[i] - 1) + sum;
}

// The swap prologue PoseidonGate and Poseidon2Gate share: wires 0..11 input, 12..23 output, 24 swap, 25..28 delta.
template <class W, class Sink>
GL_HD void swap_prologue(const W& w, Ext st[12], Sink& out) {
  const Ext swap = w(24);
  out(swap * (swap - ext(1)));
  for (int i = 0; i < 4; i++) out(swap * (w(4 + i) - w(i)) - w(25 + i));
  for (int i = 0; i < 4; i++) {
    st[i] = w(i) + w(25 + i);
    st[4 + i] = w(4 + i) - w(25 + i);
    st[8 + i] = w(8 + i);
  }
}
// a full round's S-box inputs are wires: constrain them, continue from the wires
template <class W, class Sink>
GL_HD void sbox_inputs_from_wires(const W& w, int first, Ext st[12], Sink& out) {
  for (int i = 0; i < 12; i++) {
    const Ext sb = w(first + i);
    out(st[i] - sb);
    st[i] = sb;
  }
}

// Unfiltered constraints of gate `kind` on the opened row, in the gate's constraint order.  w(i): wire i; k0, k1: the
// row's two constants (selectors stripped); pih: the public-inputs hash.
template <class W, class Sink>
GL_HD void eval_gate(uint32_t kind, const W& w, Ext k0, Ext k1, const Ext pih[4], Sink& out) {
  const Ext one = ext(1);
  switch (kind) {
    case G_CONSTANT:
      out(k0 - w(0));
      out(k1 - w(1));
      break;
    case G_PUBLIC_INPUT:
      for (int i = 0; i < 4; i++) out(w(i) - pih[i]);
      break;
    case G_BASE_SUM: {
      Ext sum = ext(0);
      for (int i = BASE_SUM_LIMBS - 1; i >= 0; i--) sum = sum * (u64)2 + w(1 + i);
      out(sum - w(0));
      for (int i = 0; i < BASE_SUM_LIMBS; i++) {
        const Ext l = w(1 + i);
        out(l * (l - one));
      }
      break;
    }
    case G_ARITHMETIC:
      for (int i = 0; i < 20; i++) out(w(4 * i + 3) - (w(4 * i) * w(4 * i + 1) * k0 + w(4 * i + 2) * k1));
      break;
    case G_MUL_EXT:
      for (int i = 0; i < 13; i++) {
        const Alg p = alg_mul(Alg{w(6 * i), w(6 * i + 1)}, Alg{w(6 * i + 2), w(6 * i + 3)});
        out(w(6 * i + 4) - p.a * k0);
        out(w(6 * i + 5) - p.b * k0);
      }
      break;
    case G_ARITH_EXT:
      for (int i = 0; i < 10; i++) {
        const Alg p = alg_mul(Alg{w(8 * i), w(8 * i + 1)}, Alg{w(8 * i + 2), w(8 * i + 3)});
        out(w(8 * i + 6) - (p.a * k0 + w(8 * i + 4) * k1));
        out(w(8 * i + 7) - (p.b * k0 + w(8 * i + 5) * k1));
      }
      break;
    case G_EXPONENTIATION: {  // wires: base 0 | power bits 1..66 | output 67 | intermediates 68..133
      const Ext base = w(0);
      for (int i = 0; i < EXP_POWER_BITS; i++) {
        Ext prev = one;
        if (i) {
          prev = w(68 + i - 1);
          prev = prev * prev;
        }
        const Ext bit = w(1 + (EXP_POWER_BITS - 1 - i));
        out(prev * (bit * base + (one - bit)) - w(68 + i));
      }
      out(w(67) - w(68 + EXP_POWER_BITS - 1));
      break;
    }
    case G_U32_ARITHMETIC:  // 3 ops: m0 m1 addend low high inverse | 32 two-bit limbs each from wire 18
      for (int op = 0; op < 3; op++) {
        const Ext m0 = w(6 * op), m1 = w(6 * op + 1), addend = w(6 * op + 2);
        const Ext lo = w(6 * op + 3), hi = w(6 * op + 4), hi_inv = w(6 * op + 5);
        out((hi_inv * (ext(0xFFFFFFFFull) - hi) - one) * lo);
        out(hi * ext((u64)1 << 32) + lo - (m0 * m1 + addend));
        Ext lo_sum = ext(0), hi_sum = ext(0);
        for (int j = 31; j >= 0; j--) {
          const Ext limb = w(18 + 32 * op + j);
          out(limb * (limb - one) * (limb - ext(2)) * (limb - ext(3)));
          if (j < 16)
            lo_sum = lo_sum * (u64)4 + limb;
          else
            hi_sum = hi_sum * (u64)4 + limb;
        }
        out(lo_sum - lo);
        out(hi_sum - hi);
      }
      break;
    case G_U32_INTERLEAVE:  // 3 ops: (x, interleaved) at 2 op | 32 big-endian bits each from wire 6
      for (int op = 0; op < 3; op++) {
        Ext x = ext(0), spread = ext(0);
        for (int bit = 0; bit < 32; bit++) {
          const Ext v = w(6 + 32 * op + bit);
          x = x * (u64)2 + v;
          spread = spread * (u64)4 + v;
        }
        out(x - w(2 * op));
        out(spread - w(2 * op + 1));
        for (int bit = 0; bit < 32; bit++) {
          const Ext v = w(6 + 32 * op + bit);
          out(v * (v - one));
        }
      }
      break;
    case G_U32_UNINTERLEAVE:  // 2 ops: (x, evens, odds) at 3 op | 64 big-endian bits each from wire 6
      for (int op = 0; op < 2; op++) {
        Ext x = ext(0), evens = ext(0), odds = ext(0);
        for (int bit = 0; bit < 64; bit++) {
          const Ext v = w(6 + 64 * op + bit);
          x = x * (u64)2 + v;
          if (bit & 1)
            odds = odds * (u64)2 + v;
          else
            evens = evens * (u64)2 + v;
        }
        out(x - w(3 * op));
        out(evens - w(3 * op + 1));
        out(odds - w(3 * op + 2));
        for (int bit = 0; bit < 64; bit++) {
          const Ext v = w(6 + 64 * op + bit);
          out(v * (v - one));
        }
      }
      break;
    case G_POSEIDON2: {  // S-box-input wires from 29 in the trace order of poseidon2.h
      Ext st[12];
      swap_prologue(w, st, out);
      p2_external(st);
      for (int r = 0; r < poseidon2::ROUND_F_BEGIN; r++) {
        for (int i = 0; i < 12; i++) st[i] = st[i] + ext(poseidon2::P2_RC[12 * r + i]);
        if (r) sbox_inputs_from_wires(w, 29 + 12 * (r - 1), st, out);
        for (int i = 0; i < 12; i++) st[i] = pow7(st[i]);
        p2_external(st);
      }
      for (int r = 0; r < poseidon2::ROUND_P; r++) {
        const Ext sb = w(29 + 36 + r);
        out(st[0] + ext(poseidon2::P2_RC_MID[r]) - sb);
        st[0] = pow7(sb);
        p2_internal(st);
      }
      for (int r = poseidon2::ROUND_F_BEGIN; r < poseidon2::ROUND_F_END; r++) {
        for (int i = 0; i < 12; i++) st[i] = st[i] + ext(poseidon2::P2_RC[12 * r + i]);
        sbox_inputs_from_wires(w, 29 + 58 + 12 * (r - poseidon2::ROUND_F_BEGIN), st, out);
        for (int i = 0; i < 12; i++) st[i] = pow7(st[i]);
        p2_external(st);
      }
      for (int i = 0; i < 12; i++) out(st[i] - w(12 + i));
      break;
    }
    case G_POSEIDON: {  // the rounds in their defining form: the constraint polynomials do not depend on the basis
      Ext st[12];
      swap_prologue(w, st, out);
      int next_wire = 29;
      for (int r = 0; r < poseidon::N_ROUNDS; r++) {
        const bool full = r < poseidon::HALF_FULL || r >= poseidon::HALF_FULL + poseidon::N_PARTIAL;
        for (int i = 0; i < 12; i++) st[i] = st[i] + ext(poseidon::RC[12 * r + i]);
        if (full) {
          if (r) {
            sbox_inputs_from_wires(w, next_wire, st, out);
            next_wire += 12;
          }
          for (int i = 0; i < 12; i++) st[i] = pow7(st[i]);
        } else {
          const Ext sb = w(next_wire++);
          out(st[0] - sb);
          st[0] = pow7(sb);
        }
        poseidon_mds(st);
      }
      for (int i = 0; i < 12; i++) out(st[i] - w(12 + i));
      break;
    }
    case G_RANDOM_ACCESS:  // per copy: index, claimed element, 16 items; the bits behind the routed wires
      for (int copy = 0; copy < RA_COPIES; copy++) {
        const int cw = (2 + RA_VEC) * copy, bw = RA_ROUTED + RA_BITS * copy;
        Ext index = ext(0);
        for (int i = 0; i < RA_BITS; i++) {
          const Ext bit = w(bw + i);
          out(bit * (bit - one));
        }
        for (int i = RA_BITS - 1; i >= 0; i--) index = index * (u64)2 + w(bw + i);
        out(index - w(cw));
        Ext items[RA_VEC];
        for (int i = 0; i < RA_VEC; i++) items[i] = w(cw + 2 + i);
        for (int level = 0, len = RA_VEC / 2; level < RA_BITS; level++, len /= 2) {
          const Ext bit = w(bw + level);
          for (int i = 0; i < len; i++) items[i] = items[2 * i] + bit * (items[2 * i + 1] - items[2 * i]);
        }
        out(items[0] - w(cw + 1));
      }
      out(k0 - w((2 + RA_VEC) * RA_COPIES));
      out(k1 - w((2 + RA_VEC) * RA_COPIES + 1));
      break;
    case G_REDUCING:
    case G_REDUCING_EXT: {  // output 0,1 | alpha 2,3 | old acc 4,5 | coefficients from 6 | accumulators behind them
      const bool ext_coeffs = kind == G_REDUCING_EXT;
      const int n_coeffs = ext_coeffs ? REDX_COEFFS : RED_COEFFS, cw = ext_coeffs ? 2 : 1, accs = 6 + n_coeffs * cw;
      const Alg alpha{w(2), w(3)};
      Alg acc{w(4), w(5)};
      for (int i = 0; i < n_coeffs; i++) {
        const int aw = i == n_coeffs - 1 ? 0 : accs + 2 * i;
        Alg t = alg_mul(acc, alpha);
        t.a = t.a + w(6 + cw * i);
        if (ext_coeffs) t.b = t.b + w(6 + cw * i + 1);
        acc = Alg{w(aw), w(aw + 1)};
        out(t.a - acc.a);
        out(t.b - acc.b);
      }
      break;
    }
    case G_POSEIDON_MDS:  // 12 algebra inputs at 0, 12 outputs at 24: the MDS layer coordinate by coordinate
      for (int r = 0; r < 12; r++)
        for (int d = 0; d < 2; d++) {
          Ext t = r == 0 ? w(d) * (u64)poseidon::MDS_DIAG0 : ext(0);
          for (int i = 0; i < 12; i++) t = t + w(2 * ((i + r) % 12) + d) * (u64)poseidon::MDS_CIRC[i];
          out(w(24 + 2 * r + d) - t);
        }
      break;
    case G_COSET_INTERP: {  // barycentric recurrence over the chunks of builder.h (ci_chunk_begin / ci_chunk_end)
      const Ext shift = w(0);
      const Alg point{w(CI_W_POINT), w(CI_W_POINT + 1)}, x{w(CI_W_SHIFTED), w(CI_W_SHIFTED + 1)};
      out(point.a - x.a * shift);
      out(point.b - x.b * shift);
      const u64 g = gl::root_of_unity(4), inv_n = gl::inv(CI_POINTS);
      Alg eval{ext(0), ext(0)}, prod{one, ext(0)};
      u64 xi = 1;
      for (int c = 0; c <= CI_INTER; c++) {
        if (c) {
          const Alg ie{w(CI_W_INTER + 2 * (c - 1)), w(CI_W_INTER + 2 * (c - 1) + 1)};
          const Alg ip{w(CI_W_INTER + 2 * CI_INTER + 2 * (c - 1)), w(CI_W_INTER + 2 * CI_INTER + 2 * (c - 1) + 1)};
          out(ie.a - eval.a);
          out(ie.b - eval.b);
          out(ip.a - prod.a);
          out(ip.b - prod.b);
          eval = ie;
          prod = ip;
        }
        const int begin = c == 0 ? 0 : 1 + (CI_DEGREE - 1) * c;
        const int stop = 1 + (CI_DEGREE - 1) * (c + 1);
        const int end = c == 0 ? CI_DEGREE : (stop < CI_POINTS ? stop : CI_POINTS);
        for (int i = begin; i < end; i++) {
          const u64 weight = gl::mul(xi, inv_n);
          const Alg v{w(1 + 2 * i) * weight, w(2 + 2 * i) * weight};
          const Alg term{x.a - ext(xi), x.b};
          const Alg e1 = alg_mul(eval, term), e2 = alg_mul(v, prod);
          eval = Alg{e1.a + e2.a, e1.b + e2.b};
          prod = alg_mul(prod, term);
          xi = gl::mul(xi, g);
        }
      }
      out(w(CI_W_VALUE) - eval.a);
      out(w(CI_W_VALUE + 1) - eval.b);
      break;
    }
    default:  // G_NOOP: no constraints
      break;
  }
}

}  // namespace extf
}  // namespace p25
