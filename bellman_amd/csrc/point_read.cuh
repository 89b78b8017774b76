// Field routines of the compressed-point reader (point_read.hip): square roots in Fp and Fp2, the "lexicographically
// largest" test of the Zcash encoding and the constants of the two endomorphism subgroup tests.  Host and device like
// the rest of ff.cuh (the host build is what tests/test_compressed_cpu.py runs through bh_test_fp_sqrt_host).
//
// p = 3 mod 4, so a square a has the root a^((p+1)/4).  The routines compute w = a^((p-3)/4) instead: r = w a is the
// candidate root, r^2 = +-a tells a square from a non-square, and 1/r = +-w comes for free - which is what lets the Fp2
// root (norm method) do without an inversion.
#pragma once
#include "ec.cuh"

namespace bh {

// ---- a^((p-3)/4) -------------------------------------------------------------------------------------------------------
// The exponent is a compile-time constant: it is cut ONCE, in a constexpr function, into a left-to-right sliding-window
// schedule over the odd powers a, a^3, a^5, a^7 - step k is sq[k] squarings followed by a product with a^dg[k] (dg = 0:
// none).  The loop that walks the schedule is the same for every lane, and the four powers are four named values
// selected by a switch on the (uniform) digit: there is no per-lane table, so nothing of it lives in scratch memory.
// 379-bit exponent: 377 squarings + 105 products + 4 for the powers (plain square-and-multiply: 378 + 227).
struct PowSchedule {
  static constexpr int MAX = 160;
  unsigned char sq[MAX] = {};
  unsigned char dg[MAX] = {};
  int n = 0;
  int first = 0;   // the leading window: the accumulator starts as a^first
};
BH_HD constexpr u32 fp_pm3d4_limb(int i) {   // limb i of (p - 3) / 4   (p = ...aaab: the low limb does not borrow)
  const u32 lo = i == 0 ? FpParams::mod(0) - 3u : FpParams::mod(i);
  const u32 hi = i < 11 ? FpParams::mod(i + 1) : 0u;
  return (lo >> 2) | (hi << 30);
}
BH_HD constexpr int fp_pm3d4_bit(int b) { return b < 0 ? 0 : (int)((fp_pm3d4_limb(b >> 5) >> (b & 31)) & 1u); }
BH_HD constexpr PowSchedule fp_pm3d4_schedule() {
  PowSchedule s;
  int i = 383;
  while (!fp_pm3d4_bit(i)) i--;
  int pending = 0;
  bool lead = true;
  while (i >= 0) {
    if (!fp_pm3d4_bit(i)) {
      pending++;
      i--;
      continue;
    }
    int len = 3;   // the longest window of at most 3 bits that ends in a set bit
    while (len > 1 && (i - len + 1 < 0 || !fp_pm3d4_bit(i - len + 1))) len--;
    int d = 0;
    for (int k = 0; k < len; k++) d = 2 * d + fp_pm3d4_bit(i - k);
    if (lead) {
      s.first = d;
      lead = false;
    } else {
      s.sq[s.n] = (unsigned char)(pending + len);
      s.dg[s.n] = (unsigned char)d;
      s.n++;
    }
    pending = 0;
    i -= len;
  }
  if (pending) {
    s.sq[s.n] = (unsigned char)pending;
    s.dg[s.n] = 0;
    s.n++;
  }
  return s;
}
// Montgomery in [0, 2p) -> a^((p-3)/4), lazily reduced; 0 -> 0
BH_HD void fp_pow_pm3d4(fp_t &r, const fp_t &a) {
  constexpr PowSchedule S = fp_pm3d4_schedule();
  static_assert(S.n > 0 && S.n < PowSchedule::MAX && (S.first & 1), "schedule of (p - 3) / 4");
  const fp_t a2 = fp_sqr_call(a);
  const fp_t a3 = fp_mul_call(a2, a), a5 = fp_mul_call(a3, a2), a7 = fp_mul_call(a5, a2);
  fp_t acc = S.first == 1 ? a : S.first == 3 ? a3 : S.first == 5 ? a5 : a7;
  for (int k = 0; k < S.n; k++) {
    for (int j = 0; j < S.sq[k]; j++) acc = fp_sqr_call(acc);
    switch (S.dg[k]) {
      case 1: acc = fp_mul_call(acc, a); break;
      case 3: acc = fp_mul_call(acc, a3); break;
      case 5: acc = fp_mul_call(acc, a5); break;
      case 7: acc = fp_mul_call(acc, a7); break;
      default: break;
    }
  }
  r = acc;
}
// r = the candidate root a^((p+1)/4), w = a^((p-3)/4); true when r^2 = a (a is a square, 0 included), else r^2 = -a.
// For a != 0: 1/r = w when a is a square, -w when it is not (r w = a^((p-1)/2) = +-1).
BH_HD bool fp_sqrt_w(fp_t &r, fp_t &w, const fp_t &a) {
  fp_pow_pm3d4(w, a);
  r = fp_mul_call(w, a);
  return fpl_eq(fp_sqr_call(r), a);
}
BH_HD bool fp_sqrt(fp_t &r, const fp_t &a) {
  fp_t w;
  return fp_sqrt_w(r, w, a);
}
// a / 2 for a in [0, 2p): (a + p) / 2 when a is odd; the result stays below 1.5 p
BH_HD void fpl_half(fp_t &r, const fp_t &a) {
  const u32 mask = 0u - (a.l[0] & 1u);
  u32 t[12], c = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) t[i] = addc(a.l[i], FpParams::mod(i) & mask, c, c);   // < 3p < 2^384
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = (t[i] >> 1) | (i < 11 ? t[i + 1] << 31 : 0u);
}
// A square root in Fp2 = Fp[u] / (u^2 + 1) by the norm: for a = a0 + a1 u with a1 != 0, s = sqrt(a0^2 + a1^2) exists
// exactly when a is a square; with t = (a0 + s) / 2 and the candidate root r of t (w = t^((p-3)/4)):
//   t a square:      root = r + (a1 / 2r) u = r + (a1 w / 2) u
//   t not a square:  r^2 = -t, and (a0 - s) / 2 = -a1^2 / 4t = (a1 / 2r)^2, so root = a1 / 2r + r u with 1/r = -w:
//                    root = -(a1 w / 2) + r u
// a1 = 0: t = a0, the same two lines give r or r u.  Two exponentiations in Fp, no inversion.  Returns false when a is not
// a square (r is then meaningless).  Every lane runs the same instruction stream.
BH_HD bool fp2_sqrt(fp2_t &r, const fp2_t &a) {
  const bool real = fpl_is_zero(a.c1);
  fp_t n, s, t, w, rt, h;
  n = fp_sqr_call(a.c0);
  t = fp_sqr_call(a.c1);
  fpl_add(n, n, t);
  const bool ok = fp_sqrt(s, n);
  fpl_add(t, a.c0, s);
  fpl_half(t, t);
  if (real) t = a.c0;
  const bool sq = fp_sqrt_w(rt, w, t);
  fpl_half(h, a.c1);
  h = fp_mul_call(h, w);
  if (sq) {
    r.c0 = rt;
    r.c1 = h;
  } else {
    fpl_neg(r.c0, h);
    r.c1 = rt;
  }
  return ok;
}

// ---- "lexicographically largest" (the sort flag of the compressed encoding) ---------------------------------------------
// y canonical Montgomery -> true when the integer y is above (p - 1) / 2
BH_HD bool fp_lex_largest(const fp_t &y_mont) {
  fp_t y;
  fe_from_mont(y, y_mont);
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {   // (p - 1) / 2 - y borrows exactly when y is larger
    const u32 half = (FpParams::mod(i) >> 1) | (i < 11 ? FpParams::mod(i + 1) << 31 : 0u);
    (void)subb(half, y.l[i], br, br);
  }
  return br != 0;
}
BH_HD bool fp2_lex_largest(const fp2_t &y_mont) {   // decided by c1, by c0 only when c1 = 0
  return fe_is_zero(y_mont.c1) ? fp_lex_largest(y_mont.c0) : fp_lex_largest(y_mont.c1);
}

// ---- constants of the endomorphism subgroup tests (M. Scott, "A note on group membership tests for G1, G2 and GT on BLS
// pairing-friendly curves", 2021), Montgomery form, little-endian 32-bit limbs; tests/test_compressed_cpu.py recomputes
// them from p.  |z| = 0xd201000000010000 is the absolute value of the curve parameter (z < 0).
//   G1: phi(x, y) = (beta x, y) equals [-z^2] P on the subgroup;  beta = 2^((p-1)/3), a cube root of unity
//   G2: psi(x, y) = (conj(x) cx, conj(y) cy) equals [z] P on the subgroup;  cx = (u+1)^(-(p-1)/3), cy = (u+1)^(-(p-1)/2)
static constexpr u64 BLS_Z_ABS = 0xd201000000010000ull;
struct EndoConsts {
  BH_HD static constexpr u32 beta(int i) {
    constexpr u32 m[12] = {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au,
                           0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu};
    return m[i];
  }
  BH_HD static constexpr u32 psi_cx(int i) {   // c0 | c1
    constexpr u32 m[24] = {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
                           0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
                           0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u,
                           0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu};
    return m[i];
  }
  BH_HD static constexpr u32 psi_cy(int i) {   // c0 | c1
    constexpr u32 m[24] = {0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du, 0x8b623732u, 0x382844c8u,
                           0x19103e18u, 0x92ad2afdu, 0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu,
                           0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u,
                           0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu};
    return m[i];
  }
};

}  // namespace bh
