// Split-scalar (GLV) point multiplication for BLS12-381 G1 and G2: r = [k] p in 128 joint double-and-add steps instead
// of the 255 of the plain ladder (point_fft.hip xyzz_mul_fr).  BH_HD like ec.cuh: the host build runs the same text
// (test_point_mul_hooks.hip, tests/cpp/glv_host_check.cpp).
//
// With z = -0xd201000000010000 and lambda = z^2 - 1 (128 bits), q = lambda^2 + lambda + 1.  Every canonical k < q is
// k = k1 + k2 lambda with k1 = k mod lambda < lambda and k2 = k div lambda <= lambda + 1: both non-negative and below
// 2^128, no lattice rounding, no signs.  (x, y) -> (c x, y) for a primitive cube root of unity c in Fp is an endomorphism
// of y^2 = x^3 + b over Fp and over Fp2; psi, the one that acts as [lambda] on the prime-order subgroup, is
//   G1: x -> beta^2 x        G2: x -> beta x        (beta = EndoConsts::beta of point_read.cuh = 2^((p-1)/3);
//                                                   tests/test_glv_cpu.py checks both against the Python reference)
// psi^2 + psi + 1 = 0 there, so P + psi P = -psi^2 P and the three nonzero entries of the joint table are free and affine:
//   (1, 0)  P = (x, y)      (0, 1)  psi P = (c x, y)      (1, 1)  P + psi P = (c' x, -y)       {c, c'} = {beta, beta^2}
// A step is one xyzz_dbl and, for a bit pair (b1, b2) != (0, 0), one mixed addition xyzz_madd of the selected entry:
// 128 x 9 + 96 x 10 = 2.11 k Fp products per G1 point with uniform scalars against 4.07 k of the ladder.
#pragma once
#include "ec.cuh"

namespace bh {

struct glv_half {
  u32 l[4];   // a 128-bit half scalar, little-endian
};

struct GlvConsts {
  BH_HD static constexpr u32 lambda(int i) {   // z^2 - 1
    constexpr u32 m[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};
    return m[i];
  }
  BH_HD static constexpr u32 mu(int i) {   // floor(2^256 / lambda), 129 bits
    constexpr u32 m[5] = {0xf6cfee30u, 0x63f6e522u, 0xe01faaddu, 0x7c6becf1u, 0x00000001u};
    return m[i];
  }
  BH_HD static constexpr u32 beta(int i) {   // Montgomery form, as EndoConsts::beta
    constexpr u32 m[12] = {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au,
                           0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu};
    return m[i];
  }
  BH_HD static constexpr u32 beta2(int i) {   // beta^2 = -beta - 1, Montgomery form
    constexpr u32 m[12] = {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu,
                           0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
    return m[i];
  }
};

// k = k1 + k2 lambda for any k < 2^255 (a canonical Fr).  Barrett with mu = floor(2^256 / lambda): qh = floor(k mu / 2^256)
// is k div lambda or one less - mu = 2^256 / lambda - e with 0 <= e < 1, so k mu / 2^256 = k / lambda - k e / 2^256 and
// k e / 2^256 < 1/2 - hence ONE conditional correction.  qh <= lambda + 1 < 2^128; the remainder before the correction
// is below 2 lambda < 2^129: five limbs.  32 x 32 -> 64-bit multiply-adds only, no division.
BH_HD void glv_split(const fr_t &k, glv_half &k1, glv_half &k2) {
  u32 prod[13];
#pragma unroll
  for (int i = 0; i < 13; i++) prod[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const u64 t = (u64)k.l[i] * GlvConsts::mu(j) + prod[i + j] + carry;
      prod[i + j] = (u32)t;
      carry = t >> 32;
    }
    prod[i + 5] = (u32)carry;
  }
  u32 qh[4];
#pragma unroll
  for (int i = 0; i < 4; i++) qh[i] = prod[8 + i];
  // the low five limbs of qh * lambda, then r = k - qh lambda mod 2^160
  u32 ql[5];
#pragma unroll
  for (int i = 0; i < 5; i++) ql[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (i + j < 5) {
        const u64 t = (u64)qh[i] * GlvConsts::lambda(j) + ql[i + j] + carry;
        ql[i + j] = (u32)t;
        carry = t >> 32;
      }
    }
    if (i == 0) ql[4] = (u32)carry;
  }
  u32 r[5], d[5];
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) r[i] = subb(k.l[i], ql[i], br, br);
  br = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) d[i] = subb(r[i], i < 4 ? GlvConsts::lambda(i) : 0u, br, br);
  const bool ge = br == 0;   // r >= lambda: the quotient was one short
  u32 c = ge ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    k1.l[i] = ge ? d[i] : r[i];
    k2.l[i] = addc(qh[i], 0u, c, c);
  }
}

// a canonical-format scalar (any 256-bit value, taken mod q as everywhere in this library) -> k < q
BH_HD void glv_reduce_canonical(fr_t &k) {
  u32 t[8];
#pragma unroll
  for (int r = 0; r < 2; r++) {   // 2^256 < 3 q
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = k.l[i];
    fe_reduce_once<FrParams>(k, t);
  }
}

template <class F>
struct GlvField;
template <>
struct GlvField<FpOps> {
  // which cube root is psi's: false = beta, true = beta^2
  static constexpr bool PSI_IS_BETA2 = true;
  // the three x coordinates live in registers beside the accumulator (36 of them; the kernel runs one wave per SIMD)
  static constexpr bool RECOMPUTE_X = false;
  BH_HD static void mul_fp(fp_t &r, const fp_t &a, const fp_t &c) { FpOps::mul(r, a, c); }
  BH_HD static void select(fp_t &r, const fp_t &a, const fp_t &b, bool pick_b) {
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = pick_b ? b.l[i] : a.l[i];
  }
};
template <>
struct GlvField<Fp2Ops> {
  static constexpr bool PSI_IS_BETA2 = false;
  // G2: three Fp2 x coordinates and -y would be 96 more registers beside a 96-register accumulator and the addition's
  // six temporaries; the selected x is recomputed at every addition instead - x times one of {1, c, c'}, 2 Fp products
  // beside the addition's 28 - and the same instruction stream serves every lane
  static constexpr bool RECOMPUTE_X = true;
  BH_HD static void mul_fp(fp2_t &r, const fp2_t &a, const fp_t &c) {
    r.c0 = fp_mul_call(a.c0, c);
    r.c1 = fp_mul_call(a.c1, c);
  }
  BH_HD static void select(fp2_t &r, const fp2_t &a, const fp2_t &b, bool pick_b) {
    GlvField<FpOps>::select(r.c0, a.c0, b.c0, pick_b);
    GlvField<FpOps>::select(r.c1, a.c1, b.c1, pick_b);
  }
};

BH_HD void glv_const(fp_t &r, bool beta2) {
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = beta2 ? GlvConsts::beta2(i) : GlvConsts::beta(i);
}

// r = [k1 + k2 lambda] p for an affine p of the prime-order subgroup and ANY 128-bit k1, k2: MSB-first over the 128 bit
// pairs, the same 128 steps in every lane (leading zero pairs double the identity: ec.cuh returns at once).  The entry is
// selected branch-free - the x coordinate among the three, y or -y - and the addition is predicated on the pair, so
// lanes with different scalars stay in one instruction stream; xyzz_madd keeps its identity / equal / opposite branches
// (a non-canonical pair can make the accumulator meet a table entry).  The identity gives the identity, (0, 0) too.
template <class F>
BH_HD void xyzz_mul_glv(XYZZ<F> &r, const Affine<F> &p, const glv_half &k1, const glv_half &k2) {
  typedef typename F::T T;
  typedef GlvField<F> G;
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  if (aff_is_identity(p)) {
    r = acc;
    return;
  }
  fp_t c_psi, c_sum;   // psi P = (c_psi x, y), P + psi P = (c_sum x, -y)
  glv_const(c_psi, G::PSI_IS_BETA2);
  glv_const(c_sum, !G::PSI_IS_BETA2);
  T x_psi, x_sum, y_neg;
  if constexpr (!G::RECOMPUTE_X) {
    G::mul_fp(x_psi, p.x, c_psi);
    G::mul_fp(x_sum, p.x, c_sum);
    F::neg(y_neg, p.y);
  }
  for (int i = 127; i >= 0; i--) {
    xyzz_dbl(acc, acc);
    const bool b1 = (k1.l[i >> 5] >> (i & 31)) & 1u, b2 = (k2.l[i >> 5] >> (i & 31)) & 1u;
    if (b1 || b2) {
      Affine<F> e;
      if constexpr (G::RECOMPUTE_X) {
        fp_t c, one;
        fe_one(one);
        GlvField<FpOps>::select(c, c_psi, c_sum, b1);   // b2 is set wherever this value is used
        GlvField<FpOps>::select(c, one, c, b2);
        G::mul_fp(e.x, p.x, c);
        F::neg(y_neg, p.y);   // (a subtraction: cheaper than 24 more live registers)
      } else {
        G::select(e.x, x_psi, x_sum, b1);
        G::select(e.x, p.x, e.x, b2);
      }
      G::select(e.y, p.y, y_neg, b1 && b2);
      xyzz_madd(acc, e);
    }
  }
  r = acc;
}

// r = [k] p for a canonical k < q
template <class F>
BH_HD void xyzz_mul_glv(XYZZ<F> &r, const Affine<F> &p, const fr_t &k) {
  glv_half k1, k2;
  glv_split(k, k1, k2);
  xyzz_mul_glv(r, p, k1, k2);
}

}  // namespace bh
