// The random linear combinations of the ceremony-step check (bh_groth16_params_verify_step, ceremony.hip): the four sums
//   S(h) = sum rho_i h_i   S(h') = sum rho_i h'_i   (coefficients of tag 4)      S(l), S(l')   (tag 5)
// over the h and l queries of two parameter sets, as ordinary multiexps over the C ABI.  a, b_g1, b_g2 must be UNCHANGED by
// a step, so they are compared byte for byte (bases_compare.cuh: no arithmetic, and the position of a difference comes for
// free); h and l are SCALED by the unknown 1/d, which no comparison can see - one combination per side and one pairing
// equation e(S(x), delta_g2) = e(S(x'), delta_g2') test x'_i = x_i / d for every i at once, with a false relation surviving
// with probability 2^-128.  The tags continue those of the transcript check (0-3, ptau_rlc.cuh), so one seed used for both
// checks gives unrelated coefficients.  Included by ceremony.hip (the product) and by test_phase2_hooks.hip (the test
// library), which runs the sums on their own: tests/test_gpu_phase2.py.
#pragma once
#include "ptau_rlc.cuh"

namespace bh {

static constexpr u32 PHASE2_TAG_H = 4, PHASE2_TAG_L = 5;

// q = h, h', l, l' (h and h' of one length, l and l' of one length): out[k] = the sum over q[k] as an affine G1 record,
// rcs[k] the code of that multiexp (BH_OK, BH_ERR_UNEXPECTED_IDENTITY when a record it consumed is the identity); an empty
// query has an empty sum: the identity record, BH_OK.  Each pair's coefficients are expanded once on `st` and shared by
// both sides; the four multiexps are issued together as ordinary jobs ordered after it (default plans: a window table is
// used where the handle has one) and waited for.  The return value carries call-level failures only.
static inline int phase2_sums(bh_ctx *ctx, const bh_bases *const q[4], const void *seed32, hipStream_t st,
                              unsigned char out[4][96], int rcs[4]) {
  void *sc[2] = {nullptr, nullptr};
  bh_msm_job *jobs[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = BH_OK;
  memset(out, 0, 4 * 96);
  for (int k = 0; k < 4; k++) rcs[k] = BH_OK;
  for (int v = 0; v < 2 && rc == BH_OK; v++) {
    const size_t terms = bh_bases_len(q[2 * v]);
    if (!terms) continue;
    rc = bh_dev_alloc(ctx, terms * 32, &sc[v]);
    if (rc == BH_OK) rc = ptau_rlc_expand(st, seed32, v == 0 ? PHASE2_TAG_H : PHASE2_TAG_L, terms, sc[v]);
  }
  for (int k = 0; k < 4 && rc == BH_OK; k++) {
    const size_t terms = bh_bases_len(q[k & ~1]);
    if (!terms) continue;
    rc = bh_msm_async_dev_after(ctx, q[k], 0, sc[k / 2], terms, BH_SCALARS_CANONICAL, nullptr, 0, nullptr, (void *)st, &jobs[k]);
  }
  for (int k = 0; k < 4; k++)   // every job issued is waited for, whatever happened to the others
    if (jobs[k]) {
      rcs[k] = bh_msm_wait(jobs[k], out[k]);
      if (rcs[k] != BH_OK && rcs[k] != BH_ERR_UNEXPECTED_IDENTITY && rc == BH_OK) rc = rcs[k];
    }
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  for (int v = 0; v < 2; v++)
    if (sc[v]) bh_dev_free(ctx, sc[v]);
  return rc;
}

}  // namespace bh
