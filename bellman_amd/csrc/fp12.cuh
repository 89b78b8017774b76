// The BLS12-381 pairing target field and the optimal-ate pairing on one lane, over Fp2Ops (ff.cuh): the Groth16
// verifier's arithmetic (groth16/src/verifier.rs:23-58, verifier/batch.rs:93-192 call it through the `pairing` crate's
// MultiMillerLoop / MillerLoopResult::final_exponentiation, which bls12_381 0.8.0 implements).
//
// Tower:  Fp6 = Fp2[v]/(v^3 - xi), xi = u + 1;   Fp12 = Fp6[w]/(w^2 - v)   (so w^6 = xi).
// An Fp12 value c0 + c1 w with ci = a + b v + c v^2 has the coefficients of w^0..w^5 c0.a, c1.a, c0.b, c1.b, c0.c, c1.c.
// All Fp values are lazily reduced in [0, 2p) like the rest of the curve code.
//
// Conventions (bls12_381 0.8.0 fixes none of these bits in what the verifier compares, see below):
//   * G2 lives on the M-type twist E': y^2 = x^3 + 4 xi, untwisted by (x, y) -> (x / w^2, y / w^3).
//   * Miller loop over |x| = 0xd201000000010000 (63 doublings, 5 additions) WITHOUT the final conjugation for x < 0:
//     f is f_{|x|,Q}(P), the inverse of the signed loop's value up to factors the final exponentiation removes.
//   * Line functions are the tangent / chord at T through P, multiplied by w^3 and by an Fp2 factor (projective
//     coordinates, no inversion): the factor lies in a proper subfield and is killed by the final exponentiation.
//   * The final exponentiation computes f^(3 (p^12 - 1) / q): easy part (p^6 - 1)(p^2 + 1), then the hard part by
//     3 (p^4 - p^2 + 1) / q = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3 (x the signed curve parameter).
//   The pairing computed here is therefore e(P, Q)^(-3) for bls12_381's e; a product of pairings is 1 here exactly when
//   it is 1 there (3 is prime to q), which is all verify_proof and the batch verifier ask.
#pragma once
#include "ff.cuh"

namespace bh {

struct alignas(16) fp6_t {
  fp2_t c[3];
};
struct alignas(16) fp12_t {
  fp6_t c0, c1;
};
// One step of the Miller loop, for a G2 point Q ("G2Prepared"): the line is l0 + (l2 * xP) w^2 + (l3 * yP) w^3
struct alignas(16) line_t {
  fp2_t l0, l2, l3;
};
static constexpr u64 BLS_X_ABS = 0xd201000000010000ull;   // |x|; x < 0
// what the verifier's launch functions (pairing_kernels.cuh) share with the units that only declare them (ceremony.hip):
// the flag bits launch_g2_lines writes per G2 point, and the most pairs one call takes (bounds the workspace: 19.6 KB of
// lines per pair)
static constexpr u32 PF_IDENTITY = 1u, PF_OFF_CURVE = 2u;
static constexpr size_t BATCH_CHUNK = 16384;
static constexpr int MILLER_LINES = 68;                    // 63 doubling + 5 addition steps

// Frobenius constants in Montgomery form (R = 2^384): FROB1[i-1] = xi^(i (p - 1) / 6) (Fp2, c0 then c1),
// FROB2[i-1] = xi^(i (p^2 - 1) / 6) (in Fp).  Computed from p; tests/test_verifier_cpu.py recomputes them.
struct FrobConsts {
  BH_HD static constexpr u32 frob1(int i, int c, int l) {
    constexpr u32 m[5][2][12] = {
        {{0xb319d465u, 0x07089552u, 0xb50a8313u, 0xc6695f92u, 0xd117228fu, 0x97e83cccu, 0xb2dc29eeu, 0xa35baecau, 0x5daace4du, 0x1ce393eau, 0xb0fb66ebu, 0x08f2220fu},
         {0x4ce5d646u, 0xb2f66aadu, 0xfc497cecu, 0x5842a06bu, 0x2599d394u, 0xcf4895d4u, 0x40a8e8d0u, 0xc11b9cbau, 0xe5a0de89u, 0x2e3813cbu, 0x88847fafu, 0x110eefdau}},
        {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
         {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u}},
        {{0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu},
         {0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}},
        {{0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu},
         {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},
        {{0x0dbce43fu, 0x82d83cf5u, 0xdf9d018fu, 0xa2813e53u, 0x3c65e181u, 0xc6f0caa5u, 0x8d50fe95u, 0x7525cf52u, 0xf4798a6bu, 0x4a85ed50u, 0x6cf8eebdu, 0x171da0fdu},
         {0xf242c66cu, 0x3726c30au, 0xd1b6fe70u, 0x7c2ac1aau, 0xba4b14a2u, 0xa04007fbu, 0x66341429u, 0xef517c32u, 0x4ed2226bu, 0x0095ba65u, 0xcc86f7ddu, 0x02e370ecu}},
    };
    return m[i][c][l];
  }
  BH_HD static constexpr u32 frob2(int i, int l) {
    constexpr u32 m[5][12] = {
        {0x798dba3au, 0xecfb361bu, 0x91865a2cu, 0xc100ddb8u, 0x232bda8eu, 0x0ec08ff1u, 0xf1ca4721u, 0xd5c13cc6u, 0xbf7b5c04u, 0x47222a47u, 0xe51c5f59u, 0x0110f184u},
        {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au, 0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu},
        {0xfffcaaaeu, 0x43f5ffffu, 0xed47fffdu, 0x32b7fff2u, 0xa2e99d69u, 0x07e83a49u, 0x8332bb7au, 0xeca8f331u, 0xa0f4c069u, 0xef148d1eu, 0x3eff0206u, 0x040ab326u},
        {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u},
        {0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu},
    };
    return m[i][l];
  }
};

typedef Fp2Ops F2;

// ---- Fp2 helpers ----------------------------------------------------------------------------------------------------
BH_HD void f2_mul_xi(fp2_t &r, const fp2_t &a) {   // a (u + 1) = (a0 - a1) + (a0 + a1) u
  fp_t t0, t1;
  fpl_sub(t0, a.c0, a.c1);
  fpl_add(t1, a.c0, a.c1);
  r.c0 = t0;
  r.c1 = t1;
}
BH_HD void f2_mul_fp(fp2_t &r, const fp2_t &a, const fp_t &b) {
  r.c0 = fp_mul_call(a.c0, b);
  r.c1 = fp_mul_call(a.c1, b);
}
BH_HD void f2_conj(fp2_t &r, const fp2_t &a) {
  r.c0 = a.c0;
  fpl_neg(r.c1, a.c1);
}

// ---- Fp6 ------------------------------------------------------------------------------------------------------------
BH_HD void f6_add(fp6_t &r, const fp6_t &a, const fp6_t &b) {
#pragma unroll
  for (int i = 0; i < 3; i++) F2::add(r.c[i], a.c[i], b.c[i]);
}
BH_HD void f6_sub(fp6_t &r, const fp6_t &a, const fp6_t &b) {
#pragma unroll
  for (int i = 0; i < 3; i++) F2::sub(r.c[i], a.c[i], b.c[i]);
}
BH_HD void f6_neg(fp6_t &r, const fp6_t &a) {
#pragma unroll
  for (int i = 0; i < 3; i++) F2::neg(r.c[i], a.c[i]);
}
BH_HD void f6_mul_v(fp6_t &r, const fp6_t &a) {   // a v
  fp2_t t;
  f2_mul_xi(t, a.c[2]);
  r.c[2] = a.c[1];
  r.c[1] = a.c[0];
  r.c[0] = t;
}
// Karatsuba / Toom-style: 6 Fp2 products
BH_HD void f6_mul(fp6_t &r, const fp6_t &a, const fp6_t &b) {
  fp2_t t0, t1, t2, s, u, r0, r1, r2;
  F2::mul(t0, a.c[0], b.c[0]);
  F2::mul(t1, a.c[1], b.c[1]);
  F2::mul(t2, a.c[2], b.c[2]);
  F2::add(s, a.c[1], a.c[2]);
  F2::add(u, b.c[1], b.c[2]);
  F2::mul(r0, s, u);
  F2::sub(r0, r0, t1);
  F2::sub(r0, r0, t2);
  f2_mul_xi(r0, r0);
  F2::add(r0, r0, t0);
  F2::add(s, a.c[0], a.c[1]);
  F2::add(u, b.c[0], b.c[1]);
  F2::mul(r1, s, u);
  F2::sub(r1, r1, t0);
  F2::sub(r1, r1, t1);
  f2_mul_xi(s, t2);
  F2::add(r1, r1, s);
  F2::add(s, a.c[0], a.c[2]);
  F2::add(u, b.c[0], b.c[2]);
  F2::mul(r2, s, u);
  F2::sub(r2, r2, t0);
  F2::sub(r2, r2, t2);
  F2::add(r2, r2, t1);
  r.c[0] = r0;
  r.c[1] = r1;
  r.c[2] = r2;
}
// a (x0 + x1 v): 5 Fp2 products
BH_HD void f6_mul_01(fp6_t &r, const fp6_t &a, const fp2_t &x0, const fp2_t &x1) {
  fp2_t t0, t1, s, u, r0, r1, r2;
  F2::mul(t0, a.c[0], x0);
  F2::mul(t1, a.c[1], x1);
  F2::add(s, a.c[0], a.c[1]);
  F2::add(u, x0, x1);
  F2::mul(r1, s, u);
  F2::sub(r1, r1, t0);
  F2::sub(r1, r1, t1);
  F2::mul(r0, a.c[2], x1);
  f2_mul_xi(r0, r0);
  F2::add(r0, r0, t0);
  F2::mul(r2, a.c[2], x0);
  F2::add(r2, r2, t1);
  r.c[0] = r0;
  r.c[1] = r1;
  r.c[2] = r2;
}
// a (y v): 3 Fp2 products
BH_HD void f6_mul_1(fp6_t &r, const fp6_t &a, const fp2_t &y) {
  fp2_t r0, r1, r2;
  F2::mul(r0, a.c[2], y);
  f2_mul_xi(r0, r0);
  F2::mul(r1, a.c[0], y);
  F2::mul(r2, a.c[1], y);
  r.c[0] = r0;
  r.c[1] = r1;
  r.c[2] = r2;
}
BH_HD void f6_inv(fp6_t &r, const fp6_t &a) {
  fp2_t t0, t1, t2, s, d;
  F2::sqr(t0, a.c[0]);
  F2::mul(s, a.c[1], a.c[2]);
  f2_mul_xi(s, s);
  F2::sub(t0, t0, s);
  F2::sqr(t1, a.c[2]);
  f2_mul_xi(t1, t1);
  F2::mul(s, a.c[0], a.c[1]);
  F2::sub(t1, t1, s);
  F2::sqr(t2, a.c[1]);
  F2::mul(s, a.c[0], a.c[2]);
  F2::sub(t2, t2, s);
  F2::mul(d, a.c[2], t1);
  F2::mul(s, a.c[1], t2);
  F2::add(d, d, s);
  f2_mul_xi(d, d);
  F2::mul(s, a.c[0], t0);
  F2::add(d, d, s);
  F2::inv(d, d);
  F2::mul(r.c[0], t0, d);
  F2::mul(r.c[1], t1, d);
  F2::mul(r.c[2], t2, d);
}

// ---- Fp12 -----------------------------------------------------------------------------------------------------------
BH_HD void f12_one(fp12_t &r) {
  F2::one(r.c0.c[0]);
  F2::zero(r.c0.c[1]);
  F2::zero(r.c0.c[2]);
#pragma unroll
  for (int i = 0; i < 3; i++) F2::zero(r.c1.c[i]);
}
BH_HD void f12_conj(fp12_t &r, const fp12_t &a) {   // a^(p^6)
  r.c0 = a.c0;
  f6_neg(r.c1, a.c1);
}
// 3 Fp6 products (54 Fp products)
BH_HD void f12_mul(fp12_t &r, const fp12_t &a, const fp12_t &b) {
  fp6_t t0, t1, s, u;
  f6_mul(t0, a.c0, b.c0);
  f6_mul(t1, a.c1, b.c1);
  f6_add(s, a.c0, a.c1);
  f6_add(u, b.c0, b.c1);
  f6_mul(s, s, u);
  f6_sub(s, s, t0);
  f6_sub(r.c1, s, t1);
  f6_mul_v(t1, t1);
  f6_add(r.c0, t0, t1);
}
// complex squaring: 2 Fp6 products (36 Fp products)
BH_HD void f12_sqr(fp12_t &r, const fp12_t &a) {
  fp6_t ab, s, u;
  f6_mul(ab, a.c0, a.c1);
  f6_add(s, a.c0, a.c1);
  f6_mul_v(u, a.c1);
  f6_add(u, a.c0, u);
  f6_mul(s, s, u);
  f6_sub(s, s, ab);
  f6_mul_v(u, ab);
  f6_sub(r.c0, s, u);
  f6_add(r.c1, ab, ab);
}
// f * (l0 + l2 w^2 + l3 w^3) = f * ((l0 + l2 v) + (l3 v) w): 13 Fp2 products (39 Fp products)
BH_HD void f12_mul_line(fp12_t &f, const fp2_t &l0, const fp2_t &l2, const fp2_t &l3) {
  fp6_t t0, t1, s;
  fp2_t x1;
  f6_mul_01(t0, f.c0, l0, l2);
  f6_mul_1(t1, f.c1, l3);
  f6_add(s, f.c0, f.c1);
  F2::add(x1, l2, l3);
  f6_mul_01(s, s, l0, x1);
  f6_sub(s, s, t0);
  f6_sub(f.c1, s, t1);
  f6_mul_v(t1, t1);
  f6_add(f.c0, t0, t1);
}
BH_HD void f12_inv(fp12_t &r, const fp12_t &a) {
  fp6_t t0, t1;
  f6_mul(t0, a.c0, a.c0);
  f6_mul(t1, a.c1, a.c1);
  f6_mul_v(t1, t1);
  f6_sub(t0, t0, t1);
  f6_inv(t0, t0);
  f6_mul(r.c0, a.c0, t0);
  f6_mul(t1, a.c1, t0);
  f6_neg(r.c1, t1);
}
// w-basis coefficient k (k = 0..5) of an Fp12 value, and the same slot for writing
BH_HD fp2_t &f12_w(fp12_t &a, int k) { return (k & 1) ? a.c1.c[k >> 1] : a.c0.c[k >> 1]; }
BH_HD const fp2_t &f12_w(const fp12_t &a, int k) { return (k & 1) ? a.c1.c[k >> 1] : a.c0.c[k >> 1]; }
// a^p: coefficient g_k of w^k -> conj(g_k) xi^(k (p - 1) / 6)
BH_HD void f12_frob1(fp12_t &r, const fp12_t &a) {
  f2_conj(r.c0.c[0], a.c0.c[0]);
#pragma unroll
  for (int k = 1; k < 6; k++) {
    fp2_t g, c;
#pragma unroll
    for (int l = 0; l < 12; l++) {
      c.c0.l[l] = FrobConsts::frob1(k - 1, 0, l);
      c.c1.l[l] = FrobConsts::frob1(k - 1, 1, l);
    }
    f2_conj(g, f12_w(a, k));
    F2::mul(f12_w(r, k), g, c);
  }
}
// a^(p^2): g_k -> g_k xi^(k (p^2 - 1) / 6), a constant in Fp
BH_HD void f12_frob2(fp12_t &r, const fp12_t &a) {
  r.c0.c[0] = a.c0.c[0];
#pragma unroll
  for (int k = 1; k < 6; k++) {
    fp_t c;
#pragma unroll
    for (int l = 0; l < 12; l++) c.l[l] = FrobConsts::frob2(k - 1, l);
    f2_mul_fp(f12_w(r, k), f12_w(a, k), c);
  }
}
// Granger-Scott squaring in the cyclotomic subgroup (the image of the easy part): 9 Fp2 squarings' worth (18 Fp products)
BH_HD void f4_sqr(fp2_t &c0, fp2_t &c1, const fp2_t &a, const fp2_t &b) {
  fp2_t t0, t1, t2;
  F2::sqr(t0, a);
  F2::sqr(t1, b);
  f2_mul_xi(t2, t1);
  F2::add(c0, t2, t0);
  F2::add(t2, a, b);
  F2::sqr(t2, t2);
  F2::sub(t2, t2, t0);
  F2::sub(c1, t2, t1);
}
BH_HD void f12_cyc_sqr(fp12_t &r, const fp12_t &f) {
  fp2_t z0 = f.c0.c[0], z4 = f.c0.c[1], z3 = f.c0.c[2], z2 = f.c1.c[0], z1 = f.c1.c[1], z5 = f.c1.c[2];
  fp2_t t0, t1, t2, t3;
  f4_sqr(t0, t1, z0, z1);
  F2::sub(z0, t0, z0);
  F2::add(z0, z0, z0);
  F2::add(z0, z0, t0);
  F2::add(z1, t1, z1);
  F2::add(z1, z1, z1);
  F2::add(z1, z1, t1);
  f4_sqr(t0, t1, z2, z3);
  f4_sqr(t2, t3, z4, z5);
  F2::sub(z4, t0, z4);
  F2::add(z4, z4, z4);
  F2::add(z4, z4, t0);
  F2::add(z5, t1, z5);
  F2::add(z5, z5, z5);
  F2::add(z5, z5, t1);
  f2_mul_xi(t0, t3);
  F2::add(z2, t0, z2);
  F2::add(z2, z2, z2);
  F2::add(z2, z2, t0);
  F2::sub(z3, t2, z3);
  F2::add(z3, z3, z3);
  F2::add(z3, z3, t2);
  r.c0.c[0] = z0; r.c0.c[1] = z4; r.c0.c[2] = z3;
  r.c1.c[0] = z2; r.c1.c[1] = z1; r.c1.c[2] = z5;
}
// f^x for f in the cyclotomic subgroup (x < 0: the conjugate of f^|x|); 63 cyclotomic squarings, 5 products
BH_HD void f12_cyc_exp_x(fp12_t &r, const fp12_t &f) {
  fp12_t acc = f;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    f12_cyc_sqr(acc, acc);
    if ((BLS_X_ABS >> i) & 1) f12_mul(acc, acc, f);
  }
  f12_conj(r, acc);
}
// f^(3 (p^12 - 1) / q), see the head of the file
BH_HD void f12_final_exp(fp12_t &r, const fp12_t &f) {
  fp12_t t, m, a, b;
  f12_inv(t, f);
  f12_conj(m, f);
  f12_mul(m, m, t);          // f^(p^6 - 1)
  f12_frob2(t, m);
  f12_mul(m, t, m);          // ^(p^2 + 1): m is in the cyclotomic subgroup from here on (inverse = conjugate)
  f12_cyc_exp_x(a, m);
  f12_conj(t, m);
  f12_mul(a, a, t);          // m^(x - 1)
  f12_cyc_exp_x(t, a);
  f12_conj(a, a);
  f12_mul(a, t, a);          // m^((x - 1)^2)
  f12_cyc_exp_x(b, a);
  f12_frob1(t, a);
  f12_mul(b, b, t);          // ^(x + p)
  f12_cyc_exp_x(a, b);
  f12_cyc_exp_x(a, a);
  f12_frob2(t, b);
  f12_mul(a, a, t);
  f12_conj(t, b);
  f12_mul(a, a, t);          // ^(x^2 + p^2 - 1)
  f12_cyc_sqr(t, m);
  f12_mul(t, t, m);
  f12_mul(r, a, t);          // * m^3
}
BH_HD bool f12_is_one(const fp12_t &a) {
  fp12_t one;
  f12_one(one);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) ok = ok && F2::eq(f12_w(a, k), f12_w(one, k));
  return ok;
}

// ---- Miller loop steps (projective T = (X : Y : Z), x = X/Z, y = Y/Z, on E': y^2 = x^3 + 4 xi) ------------------------
struct G2Proj {
  fp2_t x, y, z;
};
BH_HD void f2_mul_small(fp2_t &r, const fp2_t &a, int k) {   // r = k a for k in {3, 4, 12} by additions
  fp2_t t2, t4;
  F2::add(t2, a, a);
  if (k == 3) { F2::add(r, t2, a); return; }
  F2::add(t4, t2, t2);
  if (k == 4) { r = t4; return; }
  F2::add(t2, t4, t4);        // 8 a
  F2::add(r, t2, t4);         // 12 a
}
// T <- 2T; line = (Y^2 - 3b'Z^2, -3X^2, 2YZ): the tangent at T times 2YZ w^3
BH_HD void g2_dbl_step(G2Proj &t, line_t &l) {
  fp2_t a, b, c, e, f, h, xx, s;
  F2::mul(a, t.x, t.y);
  F2::sqr(b, t.y);
  F2::sqr(c, t.z);
  f2_mul_xi(e, c);
  f2_mul_small(e, e, 12);     // 3 b' Z^2, b' = 4 xi
  f2_mul_small(f, e, 3);
  F2::add(h, t.y, t.z);
  F2::sqr(h, h);
  F2::sub(h, h, b);
  F2::sub(h, h, c);           // 2 Y Z
  F2::sqr(xx, t.x);
  F2::sub(l.l0, b, e);
  f2_mul_small(s, xx, 3);
  F2::neg(l.l2, s);
  l.l3 = h;
  F2::add(a, a, a);
  F2::sub(s, b, f);
  F2::mul(t.x, a, s);         // X3 = 2XY (B - F)
  F2::add(s, b, f);
  F2::sqr(s, s);
  F2::sqr(e, e);
  f2_mul_small(e, e, 12);
  F2::sub(t.y, s, e);         // Y3 = (B + F)^2 - 12 E^2
  f2_mul_small(b, b, 4);
  F2::mul(t.z, b, h);         // Z3 = 4 B H
}
// T <- T + Q (Q affine); line = (th xQ - la yQ, -th, la): the chord through T and Q times la w^3
BH_HD void g2_add_step(G2Proj &t, const fp2_t &xq, const fp2_t &yq, line_t &l) {
  fp2_t th, la, c, d, e, f, g, h, s;
  F2::mul(s, yq, t.z);
  F2::sub(th, t.y, s);
  F2::mul(s, xq, t.z);
  F2::sub(la, t.x, s);
  F2::mul(c, th, xq);
  F2::mul(s, la, yq);
  F2::sub(l.l0, c, s);
  F2::neg(l.l2, th);
  l.l3 = la;
  F2::sqr(c, th);
  F2::sqr(d, la);
  F2::mul(e, la, d);
  F2::mul(f, t.z, c);
  F2::mul(g, t.x, d);
  F2::add(h, e, f);
  F2::sub(h, h, g);
  F2::sub(h, h, g);
  F2::mul(t.x, la, h);
  F2::sub(s, g, h);
  F2::mul(s, th, s);
  F2::mul(c, e, t.y);
  F2::sub(t.y, s, c);
  F2::mul(t.z, t.z, e);
}
// the 68 lines of Q (affine, not the identity), in loop order
template <class Sink>
BH_HD void g2_lines(const fp2_t &xq, const fp2_t &yq, Sink &&emit) {
  G2Proj t;
  t.x = xq;
  t.y = yq;
  F2::one(t.z);
  int k = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    line_t l;
    g2_dbl_step(t, l);
    emit(k++, l);
    if ((BLS_X_ABS >> i) & 1) {
      g2_add_step(t, xq, yq, l);
      emit(k++, l);
    }
  }
}
BH_HD void f12_mul_line_at(fp12_t &f, const line_t &l, const fp_t &xp, const fp_t &yp) {
  fp2_t l2, l3;
  f2_mul_fp(l2, l.l2, xp);
  f2_mul_fp(l3, l.l3, yp);
  f12_mul_line(f, l.l0, l2, l3);
}
// f_{|x|,Q}(P) from Q's lines; `line(k)` returns line k
template <class Lines>
BH_HD void miller_loop_lines(fp12_t &f, const fp_t &xp, const fp_t &yp, Lines &&line) {
  f12_one(f);
  int k = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    if (i != 62) f12_sqr(f, f);   // f = 1 before the first step
    f12_mul_line_at(f, line(k++), xp, yp);
    if ((BLS_X_ABS >> i) & 1) f12_mul_line_at(f, line(k++), xp, yp);
  }
}
BH_HD void f12_canon(fp12_t &a) {
#pragma unroll
  for (int k = 0; k < 6; k++) F2::canon(f12_w(a, k));
}

}  // namespace bh
