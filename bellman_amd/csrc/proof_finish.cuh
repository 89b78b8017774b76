// The tail of create_proof (prover.rs:320-360) for k proofs at once: from a proof's eight multiexp sums, the verifying
// key's five points and the blinding pair (r, s) to the three proof elements
//   A = alpha1 + [r] delta1 + a_in + a_aux                                                                  :326-327, 339-343
//   B = beta2  + [s] delta2 + b2_in + b2_aux                                                                :328-329, 347-350
//   C = [rs] delta1 + [s] alpha1 + [r] beta1 + [s] a_in + [s] a_aux + [r] b1_in + [r] b1_aux + h + l        :331-338, 351-354
// in two stages.  Stage 1 is one split-scalar multiplication (glv.cuh) per (proof, product): eight in G1, one in G2,
// results kept in XYZZ - no inversion.  The two halves of a_answer and of b_g1_answer are multiplied separately: two more
// ladders per proof, but their sum would need an inversion before it could be the affine base of a ladder.  Stage 2 is one
// lane per proof element: the additions above, one inversion, the affine record.  BH_HD like glv.cuh: the host build
// runs the same text (test_finish_hooks.hip, tests/cpp/proof_finish_host_check.hip).
// Every point is one of the prime-order subgroup (glv.cuh's ladder is only defined there): the key's points and sums of
// multiples of the CRS are.  Affine records are canonical, so the result is the bytes the host assembly writes.
#pragma once
#include "glv.cuh"

namespace bh {

typedef Affine<FpOps> pf_g1;
typedef Affine<Fp2Ops> pf_g2;

// the five points of the verifying key a proof's tail needs, in bh_groth16_params_vk's order
struct alignas(16) FinishKey {
  pf_g1 alpha_g1, beta_g1;
  pf_g2 beta_g2;
  pf_g1 delta_g1;
  pf_g2 delta_g2;
};
// BH_MSM_SUMS_BYTES: the wait order of prover.rs:339-354
struct alignas(16) FinishSums {
  pf_g1 a_in, a_aux, b1_in, b1_aux;
  pf_g2 b2_in, b2_aux;
  pf_g1 h, l;
};
struct alignas(16) FinishProof {
  pf_g1 a;
  pf_g2 b;
  pf_g1 c;
};
static_assert(sizeof(FinishKey) == 672 && sizeof(FinishSums) == 960 && sizeof(FinishProof) == 384, "record sizes");

// the G1 products of a proof, in the order of the workspace
enum FinishProduct { PF_R_DELTA, PF_RS_DELTA, PF_S_ALPHA, PF_R_BETA, PF_S_A_IN, PF_S_A_AUX, PF_R_B1_IN, PF_R_B1_AUX, PF_G1_PRODUCTS };
enum FinishElement { PF_A, PF_B, PF_C, PF_ELEMENTS };

// the canonical scalar of a product from the Montgomery pair: r, s or r s
BH_HD void finish_scalar(fr_t &k, const fr_t &r, const fr_t &s, int product) {
  fr_t m;
  if (product == PF_RS_DELTA) fe_mul(m, r, s);
  else m = (product == PF_R_DELTA || product == PF_R_BETA || product == PF_R_B1_IN || product == PF_R_B1_AUX) ? r : s;
  fe_from_mont(k, m);
}
BH_HD const pf_g1 &finish_base(const FinishKey &key, const FinishSums &sums, int product) {
  switch (product) {
    case PF_R_DELTA:
    case PF_RS_DELTA: return key.delta_g1;
    case PF_S_ALPHA: return key.alpha_g1;
    case PF_R_BETA: return key.beta_g1;
    case PF_S_A_IN: return sums.a_in;
    case PF_S_A_AUX: return sums.a_aux;
    case PF_R_B1_IN: return sums.b1_in;
    default: return sums.b1_aux;
  }
}

// stage 1, G1: product `product` of one proof
BH_HD void finish_mul_g1(XYZZ<FpOps> &out, const FinishKey &key, const FinishSums &sums, const fr_t &r, const fr_t &s, int product) {
  fr_t k;
  finish_scalar(k, r, s, product);
  const pf_g1 base = finish_base(key, sums, product);
  xyzz_mul_glv(out, base, k);
}
// stage 1, G2: [s] delta2
BH_HD void finish_mul_g2(XYZZ<Fp2Ops> &out, const FinishKey &key, const fr_t &s) {
  fr_t k;
  fe_from_mont(k, s);
  xyzz_mul_glv(out, key.delta_g2, k);
}

// acc += q for an affine q that may be the identity record (xyzz_madd takes only points)
template <class F>
BH_HD void finish_madd(XYZZ<F> &acc, const Affine<F> &q) {
  if (!aff_is_identity(q)) xyzz_madd(acc, q);
}
// stage 2: one element of one proof from the proof's products (g1: PF_G1_PRODUCTS records; g2: one)
BH_HD void finish_sum_a(pf_g1 &out, const FinishKey &key, const FinishSums &sums, const XYZZ<FpOps> *g1) {
  XYZZ<FpOps> acc = g1[PF_R_DELTA];
  finish_madd(acc, key.alpha_g1);
  finish_madd(acc, sums.a_in);
  finish_madd(acc, sums.a_aux);
  xyzz_to_affine(out, acc);
}
BH_HD void finish_sum_b(pf_g2 &out, const FinishKey &key, const FinishSums &sums, const XYZZ<Fp2Ops> &g2) {
  XYZZ<Fp2Ops> acc = g2;
  finish_madd(acc, key.beta_g2);
  finish_madd(acc, sums.b2_in);
  finish_madd(acc, sums.b2_aux);
  xyzz_to_affine(out, acc);
}
BH_HD void finish_sum_c(pf_g1 &out, const FinishSums &sums, const XYZZ<FpOps> *g1) {
  XYZZ<FpOps> acc = g1[PF_RS_DELTA];
  for (int p = PF_S_ALPHA; p < PF_G1_PRODUCTS; p++) xyzz_add(acc, acc, g1[p]);
  finish_madd(acc, sums.h);
  finish_madd(acc, sums.l);
  xyzz_to_affine(out, acc);
}

// Both stages for one proof on the host: what the kernels of proof_finish.hip compute, lane by lane.  An identity
// delta is the caller's to refuse (prover.rs:320-324).
inline void finish_proof_host(FinishProof &out, const FinishKey &key, const FinishSums &sums, const fr_t &r, const fr_t &s) {
  XYZZ<FpOps> g1[PF_G1_PRODUCTS];
  XYZZ<Fp2Ops> g2;
  for (int p = 0; p < PF_G1_PRODUCTS; p++) finish_mul_g1(g1[p], key, sums, r, s, p);
  finish_mul_g2(g2, key, s);
  finish_sum_a(out.a, key, sums, g1);
  finish_sum_b(out.b, key, sums, g2);
  finish_sum_c(out.c, sums, g1);
}

}  // namespace bh
