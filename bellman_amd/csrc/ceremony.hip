// What a receiver of a powers-of-tau transcript needs before deriving parameters from it (declared in
// include/bellman_hip.h): bh_pairing_product_is_one over arbitrary host pairs, and bh_powers_of_tau_verify - the random
// linear combination of each vector against its own shift (ptau_rlc.cuh) and six pairing equations.  And what a receiver
// of a circuit-specific contribution needs: bh_pairing_same_ratio_each (one verdict per equation e(a, B) = e(b, A): the
// contribution proofs) and bh_groth16_params_verify_step - byte comparison of everything a step must leave alone
// (bh_bases_first_difference, api_bases.hip), one linear combination per side of h and l (phase2_sums.cuh), three equations.
// And what a CONTRIBUTOR to a transcript runs: bh_powers_of_tau_contribute, four bh_bases_scale_powers (api_bases.hip; the
// split-scalar multiplier of point_mul.hip) and one host multiplication.
//
// The pairings run through the verifier's own launch functions (pairing_kernels.cuh, compiled in pairing.hip - the one
// unit of this library that includes that header - and declared in pairing_launch.hpp): the lines of every Q, one Miller lane per pair,
// the fold, the final exponentiation.  An equation e(X, Y) = e(Z, W) is evaluated as e(X, Y) e(-Z, W) == 1 on two lanes.
#include <string.h>

#include <vector>

#include "fp12.cuh"
#include "handles.hpp"
#include "pairing_launch.hpp"
#include "phase2_sums.cuh"
#include "point_read.cuh"
#include "points.hpp"
#include "ptau_rlc.cuh"

namespace bh {
namespace {

struct OwnStream {
  bh_ctx *ctx;
  void *st = nullptr;
  explicit OwnStream(bh_ctx *c) : ctx(c) {
    if (bh_stream_create(ctx, &st) != BH_OK) st = nullptr;
  }
  ~OwnStream() {
    if (st) {
      (void)hipStreamSynchronize((hipStream_t)st);
      bh_stream_destroy(ctx, st);
    }
  }
  hipStream_t get() const { return (hipStream_t)st; }
};

void neg_g1(Affine<FpOps> &r, const Affine<FpOps> &a) {
  r = a;
  if (aff_is_identity(a)) return;
  FpOps::neg(r.y, a.y);
  FpOps::canon(r.y);
}

// `lanes` pairs (p[i], q[i]) on the host.  products == 1: is_one[0] = (prod_i e(p_i, q_i) == 1).  Otherwise lanes ==
// 2 * products and is_one[k] = (e(p_k, q_k) e(p_{k + products}, q_{k + products}) == 1): the pairs fold pairwise and the
// final exponentiations run in one launch.  A pair with the identity on either side contributes 1.  *off_curve: some
// non-identity point is not on its curve (G1 tested on the host, G2 by the lines kernel); is_one is then meaningless.
int pairing_products(bh_ctx *ctx, hipStream_t st, const Affine<FpOps> *p, const Affine<Fp2Ops> *q, size_t lanes,
                     size_t products, u32 *is_one, bool *off_curve) {
  *off_curve = false;
  for (size_t i = 0; i < lanes; i++)
    if (!aff_is_identity(p[i]) && !on_curve(p[i])) *off_curve = true;
  if (*off_curve) return BH_OK;
  Context &c = ctx->c;
  const size_t bytes_p = lanes * sizeof(Affine<FpOps>), bytes_q = lanes * sizeof(Affine<Fp2Ops>);
  const size_t bytes_l = lanes * MILLER_LINES * sizeof(line_t), bytes_f = (lanes + 5 * products) * sizeof(fp12_t);
  char *d = (char *)c.pool.acquire(bytes_p + bytes_q + bytes_l + bytes_f + (lanes + products) * sizeof(u32));
  if (!d) return BH_ERR_HIP;
  Affine<FpOps> *pd = (Affine<FpOps> *)d;
  Affine<Fp2Ops> *qd = (Affine<Fp2Ops> *)(d + bytes_p);
  line_t *lines = (line_t *)(d + bytes_p + bytes_q);
  fp12_t *f = (fp12_t *)(d + bytes_p + bytes_q + bytes_l);
  fp12_t *fe = f + lanes;   // the final exponentiations' results, then 4 values of workspace each
  u32 *qflags = (u32 *)(f + lanes + 5 * products), *one_dev = qflags + lanes;
  std::vector<u32> hflags(lanes);
  int rc = BH_OK;
  if (hipMemcpyAsync(pd, p, bytes_p, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(qd, q, bytes_q, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = BH_ERR_HIP;
  if (!rc) rc = launch_g2_lines(st, qd, sizeof(Affine<Fp2Ops>), 0, lines, qflags, lanes);
  if (!rc) rc = launch_miller(st, pd, lines, qflags, f, lanes, nullptr, nullptr, 0);
  if (!rc) rc = products == 1 ? launch_fold(st, f, lanes) : launch_fold_rows(st, f, products);
  if (!rc) rc = launch_final_exp(st, f, products, fe, one_dev, fe + products);
  if (!rc && (hipMemcpyAsync(hflags.data(), qflags, lanes * sizeof(u32), hipMemcpyDeviceToHost, st) != hipSuccess ||
              hipMemcpyAsync(is_one, one_dev, products * sizeof(u32), hipMemcpyDeviceToHost, st) != hipSuccess))
    rc = BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
  c.pool.release(d);
  if (!rc)
    for (u32 fl : hflags)
      if (fl & PF_OFF_CURVE) *off_curve = true;
  return rc;
}

template <class F>
bool head_ok(const Affine<F> &p) {
  return !aff_is_identity(p) && on_curve(p);
}
}  // namespace
}  // namespace bh

using namespace bh;

extern "C" {

int bh_pairing_product_is_one(bh_ctx *ctx, const void *g1_affine_host, const void *g2_affine_host, size_t n, int *is_one) {
  if (!ctx || !is_one || (n && (!g1_affine_host || !g2_affine_host)) || n > BATCH_CHUNK) return BH_ERR_INVALID_ARG;
  *is_one = 0;
  if (!n) {
    *is_one = 1;
    return BH_OK;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  OwnStream own(ctx);
  if (!own.st) return BH_ERR_HIP;
  u32 one = 0;
  bool off = false;
  const int rc = pairing_products(ctx, own.get(), (const Affine<FpOps> *)g1_affine_host, (const Affine<Fp2Ops> *)g2_affine_host,
                                  n, 1, &one, &off);
  if (rc) return rc;
  if (off) return BH_ERR_INVALID_POINT;
  *is_one = one == 1;
  return BH_OK;
}

int bh_powers_of_tau_verify(bh_ctx *ctx, const bh_powers_of_tau *t, const void *seed32, unsigned flags, bh_ptau_report *report) {
  bh_ptau_report local;
  bh_ptau_report &rep = report ? *report : local;
  rep.failed = 0;
  rep.bad_vector = 0;
  rep.bad_index = 0;
  if (!ctx || !t || !seed32 || !t->tau_g1 || !t->tau_g2 || !t->alpha_tau_g1 || !t->beta_tau_g1 || !t->beta_g2 ||
      (flags & ~BH_PTAU_VALIDATE_POINTS))
    return BH_ERR_INVALID_ARG;
  const bh_bases *vec[4] = {t->tau_g1, t->tau_g2, t->alpha_tau_g1, t->beta_tau_g1};
  static const size_t min_len[4] = {2, 2, 1, 1};
  for (int v = 0; v < 4; v++)
    if (vec[v]->group != (v == 1 ? BH_G2 : BH_G1) || bh_bases_len(vec[v]) < min_len[v]) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));

  if (flags & BH_PTAU_VALIDATE_POINTS)
    for (int v = 0; v < 4; v++) {
      size_t bad = 0;
      const int rc = bh_bases_validate(ctx, vec[v], 0, bh_bases_len(vec[v]), BH_POINTS_CHECKED | BH_POINTS_FORBID_IDENTITY,
                                       nullptr, &bad);
      if (rc == BH_ERR_INVALID_POINT || rc == BH_ERR_POINT_AT_INFINITY) {
        rep.failed = BH_PTAU_FAILED_POINTS;
        rep.bad_vector = (uint32_t)v;
        rep.bad_index = bad;
      }
      if (rc) return rc;
    }

  OwnStream own(ctx);
  if (!own.st) return BH_ERR_HIP;
  hipStream_t st = own.get();
  // the head points: g1, s1 = T[0], T[1]; g2, s2 = U[0], U[1]; A[0]; B[0]; beta_g2
  Affine<FpOps> g1, s1, a0, b0;
  Affine<Fp2Ops> g2, s2, beta2;
  {
    char *stage = (char *)ctx->c.pool.acquire(4 * 96 + 2 * 192);
    if (!stage) return BH_ERR_HIP;
    int rc = bh_bases_copy_out_dev(ctx, vec[0], BH_G1, 0, 2, stage, st);
    if (!rc) rc = bh_bases_copy_out_dev(ctx, vec[2], BH_G1, 0, 1, stage + 192, st);
    if (!rc) rc = bh_bases_copy_out_dev(ctx, vec[3], BH_G1, 0, 1, stage + 288, st);
    if (!rc) rc = bh_bases_copy_out_dev(ctx, vec[1], BH_G2, 0, 2, stage + 384, st);
    unsigned char h[4 * 96 + 2 * 192];
    if (!rc && hipMemcpyAsync(h, stage, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess) rc = BH_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
    ctx->c.pool.release(stage);
    if (rc) return rc;
    memcpy(&g1, h, 96);
    memcpy(&s1, h + 96, 96);
    memcpy(&a0, h + 192, 96);
    memcpy(&b0, h + 288, 96);
    memcpy(&g2, h + 384, 192);
    memcpy(&s2, h + 576, 192);
    memcpy(&beta2, t->beta_g2, 192);
  }
  if (!head_ok(g1) || !head_ok(s1) || !head_ok(a0) || !head_ok(b0) || !head_ok(g2) || !head_ok(s2) || !head_ok(beta2)) {
    rep.failed = BH_PTAU_FAILED_HEAD;
    return BH_ERR_INVALID_TRANSCRIPT;
  }

  alignas(16) unsigned char sums[8][192];
  int rcs[8];
  int rc = ptau_sums(ctx, vec, seed32, st, sums, rcs);
  if (rc) return rc;
  static const uint32_t vec_bit[4] = {BH_PTAU_FAILED_TAU_G1, BH_PTAU_FAILED_TAU_G2, BH_PTAU_FAILED_ALPHA, BH_PTAU_FAILED_BETA};
  bool skip_eq[4];
  for (int v = 0; v < 4; v++) {
    const bool ident = rcs[2 * v] == BH_ERR_UNEXPECTED_IDENTITY || rcs[2 * v + 1] == BH_ERR_UNEXPECTED_IDENTITY;
    if (ident) rep.failed |= vec_bit[v];   // no consistent transcript holds an identity
    skip_eq[v] = ident || bh_bases_len(vec[v]) == 1;   // (one point: no relation to check)
  }

  // the equations e(X, Y) = e(Z, W) as lanes (X, Y) and (-Z, W)
  Affine<FpOps> px[6], pz[6];
  Affine<Fp2Ops> qy[6], qw[6];
  uint32_t bit[6];
  size_t m = 0;
  auto equation = [&](uint32_t b, const Affine<FpOps> &x, const Affine<Fp2Ops> &y, const Affine<FpOps> &z, const Affine<Fp2Ops> &w) {
    bit[m] = b;
    px[m] = x;
    qy[m] = y;
    neg_g1(pz[m], z);
    qw[m] = w;
    m++;
  };
  Affine<FpOps> P1[4], Q1[4];   // the G1 sums (index 1 unused)
  Affine<Fp2Ops> PU, QU;
  for (int v = 0; v < 4; v++) {
    if (v == 1) continue;
    memcpy(&P1[v], sums[2 * v], 96);
    memcpy(&Q1[v], sums[2 * v + 1], 96);
  }
  memcpy(&PU, sums[2], 192);
  memcpy(&QU, sums[3], 192);
  equation(BH_PTAU_FAILED_TAU_G1_G2, s1, g2, g1, s2);
  if (!skip_eq[0]) equation(BH_PTAU_FAILED_TAU_G1, P1[0], s2, Q1[0], g2);
  if (!skip_eq[1]) equation(BH_PTAU_FAILED_TAU_G2, s1, PU, g1, QU);
  if (!skip_eq[2]) equation(BH_PTAU_FAILED_ALPHA, P1[2], s2, Q1[2], g2);
  if (!skip_eq[3]) equation(BH_PTAU_FAILED_BETA, P1[3], s2, Q1[3], g2);
  equation(BH_PTAU_FAILED_BETA_G2, b0, g2, g1, beta2);
  Affine<FpOps> p[12];
  Affine<Fp2Ops> q[12];
  for (size_t k = 0; k < m; k++) {
    p[k] = px[k];
    q[k] = qy[k];
    p[m + k] = pz[k];
    q[m + k] = qw[k];
  }
  u32 one[6] = {0, 0, 0, 0, 0, 0};
  bool off = false;
  rc = pairing_products(ctx, st, p, q, 2 * m, m, one, &off);
  if (rc) return rc;
  if (off) return BH_ERR_INVALID_POINT;   // a multiexp over records that are not on the curve (validate the points)
  for (size_t k = 0; k < m; k++)
    if (one[k] != 1) rep.failed |= bit[k];
  return rep.failed ? BH_ERR_INVALID_TRANSCRIPT : BH_OK;
}

int bh_powers_of_tau_contribute(bh_ctx *ctx, const bh_powers_of_tau *before, const void *tau_mont, const void *alpha_mont,
                                const void *beta_mont, bh_bases *out[4], void *beta_g2_out) {
  if (!ctx || !before || !tau_mont || !alpha_mont || !beta_mont || !out || !beta_g2_out || !before->tau_g1 || !before->tau_g2 ||
      !before->alpha_tau_g1 || !before->beta_tau_g1 || !before->beta_g2)
    return BH_ERR_INVALID_ARG;
  const bh_bases *vec[4] = {before->tau_g1, before->tau_g2, before->alpha_tau_g1, before->beta_tau_g1};
  for (int v = 0; v < 4; v++) {
    out[v] = nullptr;
    if (vec[v]->group != (v == 1 ? BH_G2 : BH_G1)) return BH_ERR_INVALID_ARG;
  }
  fr_t secret[3], canon[3], one;   // tau, alpha, beta
  const void *src[3] = {tau_mont, alpha_mont, beta_mont};
  for (int k = 0; k < 3; k++) {
    memcpy(&secret[k], src[k], sizeof(fr_t));
    fe_from_mont(canon[k], secret[k]);
    if (fe_is_zero(canon[k])) return BH_ERR_UNEXPECTED_IDENTITY;
  }
  fe_one(one);
  const fr_t *scale[4] = {&one, &one, &secret[1], &secret[2]};
  for (int v = 0; v < 4; v++) {   // each on a stream of its own (bh_bases_scale_powers)
    const int rc = bh_bases_scale_powers(ctx, vec[v], scale[v], &secret[0], &out[v]);
    if (rc) {
      for (int w = 0; w < v; w++) {
        bh_bases_release(ctx, out[w]);
        out[w] = nullptr;
      }
      return rc;
    }
  }
  Affine<Fp2Ops> b2, r2;
  memcpy(&b2, before->beta_g2, sizeof b2);
  bh_point_mul(BH_G2, &r2, &b2, &canon[2]);
  memcpy(beta_g2_out, &r2, sizeof r2);
  return BH_OK;
}

int bh_pairing_same_ratio_each(bh_ctx *ctx, const void *a_g1, const void *b_g1, const void *A_g2, const void *B_g2, size_t n,
                               int32_t *verdicts, size_t *n_bad) {
  if (!ctx || (n && (!a_g1 || !b_g1 || !A_g2 || !B_g2 || !verdicts))) return BH_ERR_INVALID_ARG;
  if (n_bad) *n_bad = 0;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  OwnStream own(ctx);
  if (!own.st) return BH_ERR_HIP;
  constexpr size_t ROWS = BATCH_CHUNK / 2;
  const size_t ch = n < ROWS ? n : ROWS;
  std::vector<Affine<FpOps>> p(2 * ch);
  std::vector<Affine<Fp2Ops>> q(2 * ch);
  std::vector<u32> one(ch);
  size_t bad = 0;
  for (size_t off = 0; off < n; off += ch) {
    const size_t m = n - off < ch ? n - off : ch;
    // row k of the chunk: lanes k = (a, B) and m + k = (-b, A); a row decided here keeps both lanes, as identity pairs
    for (size_t k = 0; k < m; k++) {
      Affine<FpOps> a, b;
      Affine<Fp2Ops> A, B;
      memcpy(&a, (const char *)a_g1 + (off + k) * 96, 96);
      memcpy(&b, (const char *)b_g1 + (off + k) * 96, 96);
      memcpy(&A, (const char *)A_g2 + (off + k) * 192, 192);
      memcpy(&B, (const char *)B_g2 + (off + k) * 192, 192);
      int32_t v = BH_OK;
      if (aff_is_identity(a) || aff_is_identity(b) || aff_is_identity(A) || aff_is_identity(B))
        v = BH_ERR_POINT_AT_INFINITY;
      else if (!on_curve(a) || !on_curve(b) || !on_curve(A) || !on_curve(B))
        v = BH_ERR_INVALID_POINT;
      verdicts[off + k] = v;
      if (v != BH_OK) {
        memset(&p[k], 0, 96);
        memset(&p[m + k], 0, 96);
        memset(&q[k], 0, 192);
        memset(&q[m + k], 0, 192);
      } else {
        p[k] = a;
        q[k] = B;
        neg_g1(p[m + k], b);
        q[m + k] = A;
      }
    }
    bool off_curve = false;
    const int rc = pairing_products(ctx, own.get(), p.data(), q.data(), 2 * m, m, one.data(), &off_curve);
    if (rc) return rc;
    if (off_curve) return BH_ERR_HIP;   // (every point was tested above: the device disagrees with the host)
    for (size_t k = 0; k < m; k++) {
      if (verdicts[off + k] == BH_OK && one[k] != 1) verdicts[off + k] = BH_ERR_INVALID_TRANSCRIPT;
      if (verdicts[off + k] != BH_OK) bad++;
    }
  }
  if (n_bad) *n_bad = bad;
  return BH_OK;
}

int bh_groth16_params_verify_step(bh_ctx *ctx, const bh_params *before, const bh_params *after, const void *seed32,
                                  unsigned flags, bh_params_step_report *report) {
  bh_params_step_report local;
  bh_params_step_report &rep = report ? *report : local;
  rep.failed = 0;
  rep.bad_vector = 0;
  rep.bad_index = 0;
  if (!ctx || !before || !after || !seed32 || (flags & ~BH_STEP_VALIDATE_POINTS)) return BH_ERR_INVALID_ARG;
  // which = 0 h, 1 l, 2 a, 3 b_g1, 4 b_g2; side 0 = before, 1 = after
  const bh_params *side[2] = {before, after};
  const bh_bases *qv[2][5];
  size_t n_ic[2] = {0, 0};
  for (int s = 0; s < 2; s++) {
    for (int w = 0; w < 5; w++) {
      const int rc = bh_groth16_params_query(side[s], w, &qv[s][w], nullptr);
      if (rc) return rc;
      if (!qv[s][w] || qv[s][w]->group != (w == 4 ? BH_G2 : BH_G1)) return BH_ERR_INVALID_ARG;
    }
    const int rc = bh_groth16_params_vk_ext(side[s], nullptr, nullptr, 0, &n_ic[s]);
    if (rc) return rc;
  }
  bool shape = n_ic[0] != n_ic[1];
  for (int w = 0; w < 5; w++) shape = shape || bh_bases_len(qv[0][w]) != bh_bases_len(qv[1][w]);
  if (shape) {
    rep.failed = BH_STEP_FAILED_SHAPE;
    return BH_ERR_INVALID_TRANSCRIPT;
  }
  // the key elements: alpha_g1, beta_g1, beta_g2, gamma_g2, ic compared; delta_g1, delta_g2 related by the equations
  Affine<FpOps> alpha[2], beta1[2], delta1[2];
  Affine<Fp2Ops> beta2[2], gamma2[2], delta2[2];
  std::vector<Affine<FpOps>> ic[2];
  for (int s = 0; s < 2; s++) {
    ic[s].resize(n_ic[s]);
    int rc = bh_groth16_params_vk(side[s], &alpha[s], &beta1[s], &beta2[s], &delta1[s], &delta2[s]);
    if (!rc) rc = bh_groth16_params_vk_ext(side[s], &gamma2[s], n_ic[s] ? ic[s].data() : nullptr, n_ic[s], nullptr);
    if (rc) return rc;
  }
  if (!head_ok(delta1[0]) || !head_ok(delta1[1]) || !head_ok(delta2[0]) || !head_ok(delta2[1])) {
    rep.failed = BH_STEP_FAILED_HEAD;
    return BH_ERR_INVALID_TRANSCRIPT;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));

  if (flags & BH_STEP_VALIDATE_POINTS) {
    const unsigned vflags = BH_POINTS_CHECKED | BH_POINTS_FORBID_IDENTITY;
    auto points_failed = [&](int rc, uint32_t vector, size_t index) {
      if (rc == BH_ERR_INVALID_POINT || rc == BH_ERR_POINT_AT_INFINITY) {
        rep.failed = BH_STEP_FAILED_POINTS;
        rep.bad_vector = vector;
        rep.bad_index = index;
      }
      return rc;
    };
    for (int w = 0; w < 2; w++) {
      size_t bad = 0;
      const int rc = bh_bases_validate(ctx, qv[1][w], 0, bh_bases_len(qv[1][w]), vflags, nullptr, &bad);
      if (rc) return points_failed(rc, 4 + (uint32_t)w, bad);
    }
    for (int g = 0; g < 2; g++) {   // delta_g1', delta_g2': one-record views of a staging buffer
      const int group = g == 0 ? BH_G1 : BH_G2;
      const size_t rec = g == 0 ? 96 : 192;
      void *stage = nullptr;
      bh_bases *one = nullptr;
      int rc = bh_dev_alloc(ctx, rec, &stage);
      if (rc) return rc;
      rc = bh_dev_upload(ctx, stage, g == 0 ? (const void *)&delta1[1] : (const void *)&delta2[1], rec);
      if (!rc) rc = bh_bases_wrap_dev(ctx, group, stage, 1, &one);
      if (!rc) rc = bh_bases_validate(ctx, one, 0, 1, vflags, nullptr, nullptr);
      if (one) bh_bases_release(ctx, one);
      bh_dev_free(ctx, stage);
      if (rc) return points_failed(rc, 6 + (uint32_t)g, 0);
    }
  }

  bool placed = false;   // bad_vector / bad_index name the first finding that has a position
  auto finding = [&](uint32_t bit, uint32_t vector, size_t index) {
    rep.failed |= bit;
    if (!placed) {
      rep.bad_vector = vector;
      rep.bad_index = index;
      placed = true;
    }
  };
  if (memcmp(&alpha[0], &alpha[1], 96)) finding(BH_STEP_FAILED_KEY, 0, 0);
  if (memcmp(&beta1[0], &beta1[1], 96)) finding(BH_STEP_FAILED_KEY, 0, 1);
  if (memcmp(&beta2[0], &beta2[1], 192)) finding(BH_STEP_FAILED_KEY, 0, 2);
  if (memcmp(&gamma2[0], &gamma2[1], 192)) finding(BH_STEP_FAILED_KEY, 0, 3);
  for (size_t i = 0; i < n_ic[0]; i++)
    if (memcmp(&ic[0][i], &ic[1][i], 96)) {
      finding(BH_STEP_FAILED_KEY, 0, 4 + i);
      break;
    }
  static const uint32_t same_bit[3] = {BH_STEP_FAILED_A, BH_STEP_FAILED_B_G1, BH_STEP_FAILED_B_G2};
  for (int w = 2; w < 5; w++) {
    const size_t len = bh_bases_len(qv[0][w]);
    size_t at = len;
    const int rc = bh_bases_first_difference(ctx, qv[0][w], 0, qv[1][w], 0, len, &at);
    if (rc) return rc;
    if (at != len) finding(same_bit[w - 2], (uint32_t)(w - 1), at);
  }

  OwnStream own(ctx);
  if (!own.st) return BH_ERR_HIP;
  hipStream_t st = own.get();
  const bh_bases *sq[4] = {qv[0][0], qv[1][0], qv[0][1], qv[1][1]};
  alignas(16) unsigned char sums[4][96];
  int rcs[4];
  int rc = phase2_sums(ctx, sq, seed32, st, sums, rcs);
  if (rc) return rc;
  static const uint32_t sum_bit[2] = {BH_STEP_FAILED_H, BH_STEP_FAILED_L};
  bool skip_eq[2];
  for (int v = 0; v < 2; v++) {
    const bool ident = rcs[2 * v] == BH_ERR_UNEXPECTED_IDENTITY || rcs[2 * v + 1] == BH_ERR_UNEXPECTED_IDENTITY;
    if (ident) rep.failed |= sum_bit[v];   // no honest query holds an identity
    skip_eq[v] = ident || bh_bases_len(sq[2 * v]) == 0;
  }
  // the equations e(X, Y) = e(Z, W) as lanes (X, Y) and (-Z, W)
  Affine<FpOps> p[6];
  Affine<Fp2Ops> q[6];
  Affine<FpOps> px[3], pz[3];
  Affine<Fp2Ops> qy[3], qw[3];
  uint32_t bit[3];
  size_t m = 0;
  auto equation = [&](uint32_t b, const Affine<FpOps> &x, const Affine<Fp2Ops> &y, const Affine<FpOps> &z, const Affine<Fp2Ops> &w) {
    bit[m] = b;
    px[m] = x;
    qy[m] = y;
    neg_g1(pz[m], z);
    qw[m] = w;
    m++;
  };
  equation(BH_STEP_FAILED_DELTA, delta1[1], delta2[0], delta1[0], delta2[1]);
  for (int v = 0; v < 2; v++) {
    if (skip_eq[v]) continue;
    Affine<FpOps> s0, s1;
    memcpy(&s0, sums[2 * v], 96);
    memcpy(&s1, sums[2 * v + 1], 96);
    equation(sum_bit[v], s0, delta2[0], s1, delta2[1]);
  }
  for (size_t k = 0; k < m; k++) {
    p[k] = px[k];
    q[k] = qy[k];
    p[m + k] = pz[k];
    q[m + k] = qw[k];
  }
  u32 one[3] = {0, 0, 0};
  bool off = false;
  rc = pairing_products(ctx, st, p, q, 2 * m, m, one, &off);
  if (rc) return rc;
  if (off) return BH_ERR_INVALID_POINT;   // a multiexp over records that are not on the curve (validate the points)
  for (size_t k = 0; k < m; k++)
    if (one[k] != 1) rep.failed |= bit[k];
  return rep.failed ? BH_ERR_INVALID_TRANSCRIPT : BH_OK;
}

}  // extern "C"
