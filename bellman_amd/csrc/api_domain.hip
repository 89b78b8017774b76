// EvaluationDomain over Fr and over G1 / G2 points: entry points of include/bellman_hip.h, with the rules that send
// a call over k vectors to the batched launches or to k single-vector transforms.
#include <string.h>

#include "fft.hpp"
#include "handles.hpp"
#include "point_ops.hpp"

using namespace bh;

extern "C" {

// ---- EvaluationDomain ------------------------------------------------------------------------
int bh_fft_fr_dev(bh_ctx *ctx, void *data_dev, uint32_t log_n, int mode, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = nullptr;
  if (log_n > 11) {   // more than one pass (fft.hip NTT_MAX_R)
    scratch = ctx->c.pool.acquire(sizeof(fr_t) << log_n);
    if (!scratch) return BH_ERR_HIP;
  }
  int rc = ntt_run(ctx->c, (fr_t *)data_dev, (fr_t *)scratch, log_n, mode, st);
  if (scratch) {
    // the scratch buffer may be recycled by another stream: fence before returning it
    if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
    ctx->c.pool.release(scratch);
  }
  return rc;
}
int bh_fft_fr(bh_ctx *ctx, void *data_host, uint32_t log_n, int mode) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  const size_t bytes = sizeof(fr_t) << log_n;
  void *d = ctx->c.pool.acquire(bytes);
  if (!d) return BH_ERR_HIP;
  int rc = bh_dev_upload(ctx, d, data_host, bytes);
  if (rc == BH_OK) rc = bh_fft_fr_dev(ctx, d, log_n, mode, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, data_host, d, bytes);
  ctx->c.pool.release(d);
  return rc;
}
// ---- k vectors per call (fft.hip ntt_run_many) ------------------------------------------------------------------
// Where the batched launches replace k single-vector transforms without being asked to (BH_FFT_MANY_FORCE).  Set from
// profiles/fft_many_bench.json (tools/bench_fft_many.py): a shape is taken only where the batched call's min-of-5 wall time
// is below the baseline's by more than the baseline's own spread in that run.  Shapes nobody measured take the single path.
// Measured (MI355X, 2^6 ... 2^22 points in steps of 4x, k = 2, 4, 16, 64 with k * n <= 2^24; ifft at every k, the four modes
// at k = 4, the h block at every k):
//   transforms  win at every measured shape from 2^6 to 2^20 (2^8 x 64: 0.050 ms against 1.68; 2^16 x 4: 0.069 against
//               0.25; 2^20 x 16: 1.65 against 2.16) and not at 2^22 (0.97 - 1.01 x; one shape of five, coset_fft x 4, is 1 %
//               beyond the spread in one run of two: the passes fill the chip by themselves, and the table entries a
//               group of vectors could share are not what bounds them);
//   h blocks    win from 2^12 to 2^20 at every k (2^14 x 4: 0.36 ms against 1.37), from 2^6 to 2^10 at k >= 4 only (at k = 2
//               the single h block's own three-vector launches are 0.16 - 0.22 ms against 0.22 - 0.34), and not at 2^22
//               (0.91 - 0.96 x).
// The rule covers the measured box and what lies between its points (odd log_n, k = 3, 5 ... 63).  Outside it - fewer than
// 2^6 or more than 2^20 points, k = 1, k > 64, more than 2^24 elements in all - the call issues single-vector transforms.
constexpr uint32_t FFT_MANY_RULE_LOG_N_MIN = 6, FFT_MANY_RULE_LOG_N_MAX = 20, FFT_MANY_RULE_LOG_ELEMS_MAX = 24;
constexpr size_t FFT_MANY_RULE_K_MIN = 2, FFT_MANY_RULE_K_MAX = 64, FFT_MANY_RULE_H_SMALL_K_MIN = 4;
static bool fft_many_wins(uint32_t log_n, size_t k, bool h_block = false) {
  if (log_n < FFT_MANY_RULE_LOG_N_MIN || log_n > FFT_MANY_RULE_LOG_N_MAX || k < FFT_MANY_RULE_K_MIN || k > FFT_MANY_RULE_K_MAX) return false;
  if ((k << log_n) > ((size_t)1 << FFT_MANY_RULE_LOG_ELEMS_MAX)) return false;
  if (h_block && log_n <= 11 && k < FFT_MANY_RULE_H_SMALL_K_MIN) return false;
  return true;
}
// the checks the four calls share; *use_many: batched launches or k single-vector transforms
static int fft_many_args(bh_ctx *ctx, const void *data, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                         bool *use_many, bool h_block = false) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !data || mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  if (stride_bytes < ((size_t)sizeof(fr_t) << log_n) || stride_bytes % sizeof(fr_t)) return BH_ERR_INVALID_ARG;
  if ((flags & ~(unsigned)(BH_FFT_MANY_FORCE | BH_FFT_MANY_SINGLE)) || flags == (BH_FFT_MANY_FORCE | BH_FFT_MANY_SINGLE))
    return BH_ERR_INVALID_ARG;
  *use_many = (flags & BH_FFT_MANY_FORCE) || (!(flags & BH_FFT_MANY_SINGLE) && fft_many_wins(log_n, k, h_block));
  return BH_OK;
}
static bool fft_many_scratch_ok(uint32_t log_n, const void *scratch, size_t scratch_bytes) {
  return log_n <= 11 || (scratch && scratch_bytes >= ((size_t)sizeof(fr_t) << log_n));
}
int bh_fft_fr_many_dev_on(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                          void *scratch_dev, size_t scratch_bytes, void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, data_dev, stride_bytes, k, log_n, mode, flags, &use_many);
  if (rc) return rc;
  if (!fft_many_scratch_ok(log_n, scratch_dev, scratch_bytes)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  const u64 stride = stride_bytes / sizeof(fr_t);
  if (!use_many) return ntt_run_each(ctx->c, (fr_t *)data_dev, stride, k, log_n, mode, (fr_t *)scratch_dev, st);
  return ntt_run_many(ctx->c, (fr_t *)data_dev, stride, k, log_n, mode, (fr_t *)scratch_dev, scratch_bytes >> (log_n + 5), st);
}
int bh_fft_fr_many_dev(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                       void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, data_dev, stride_bytes, k, log_n, mode, flags, &use_many);
  if (rc || !k) return rc;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  if (log_n > 11) {
    // a scratch vector per transformed vector, up to 256 MiB; one vector where the pool cannot give more
    const size_t one = sizeof(fr_t) << log_n;
    size_t vecs = use_many ? k : 1;
    while (vecs > 1 && vecs * one > ((size_t)256 << 20)) vecs = (vecs + 1) / 2;
    scratch = ctx->c.pool.acquire(vecs * one);
    if (!scratch && vecs > 1) { vecs = 1; scratch = ctx->c.pool.acquire(one); }
    if (!scratch) return BH_ERR_HIP;
    scratch_bytes = vecs * one;
  }
  rc = bh_fft_fr_many_dev_on(ctx, data_dev, stride_bytes, k, log_n, mode, flags, scratch, scratch_bytes, stream);
  if (scratch) {
    // the scratch buffer may be recycled by another stream: fence before returning it
    if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
    ctx->c.pool.release(scratch);
  }
  return rc;
}
int bh_fft_fr_many(bh_ctx *ctx, void *data_host, size_t k, uint32_t log_n, int mode) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !data_host || mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  const size_t one = sizeof(fr_t) << log_n, bytes = one * k;
  void *d = ctx->c.pool.acquire(bytes);
  if (!d) return BH_ERR_HIP;
  int rc = bh_dev_upload(ctx, d, data_host, bytes);
  if (rc == BH_OK) rc = bh_fft_fr_many_dev(ctx, d, one, k, log_n, mode, 0, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, data_host, d, bytes);
  ctx->c.pool.release(d);
  return rc;
}
int bh_h_poly_fr_many_dev_on(bh_ctx *ctx, void *a, void *b, void *c, size_t stride_bytes, size_t k, uint32_t log_n, unsigned flags,
                             void *scratch_dev, size_t scratch_bytes, void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, a, stride_bytes, k, log_n, BH_FFT, flags, &use_many, true);
  if (rc) return rc;
  if (!b || !c || !fft_many_scratch_ok(log_n, scratch_dev, scratch_bytes)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  const u64 stride = stride_bytes / sizeof(fr_t);
  if (!use_many) return h_poly_each_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, stride, k, log_n, (fr_t *)scratch_dev, st);
  return h_poly_many_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, stride, k, log_n, (fr_t *)scratch_dev, scratch_bytes >> (log_n + 5), st);
}
int bh_fr_mul_assign_dev(bh_ctx *ctx, void *a, const void *b, size_t n, void *stream) {
  return fr_mul_assign(ctx->c, (fr_t *)a, (const fr_t *)b, n, pick_stream(ctx, stream));
}
int bh_fr_sub_assign_dev(bh_ctx *ctx, void *a, const void *b, size_t n, void *stream) {
  return fr_sub_assign(ctx->c, (fr_t *)a, (const fr_t *)b, n, pick_stream(ctx, stream));
}
int bh_fr_divide_by_z_on_coset_dev(bh_ctx *ctx, void *a, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  return fr_divide_by_z(ctx->c, (fr_t *)a, log_n, pick_stream(ctx, stream));
}
int bh_fr_distribute_powers_dev(bh_ctx *ctx, void *a, size_t n, const void *g_host, void *stream) {
  fr_t g;
  memcpy(&g, g_host, sizeof g);
  return fr_distribute_powers(ctx->c, (fr_t *)a, n, g, pick_stream(ctx, stream));
}
// ---- EvaluationDomain<Fr, Point<G>> (point_fft.hip) ----------------------------------------------
int bh_fft_point_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, int mode, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !group_ok(group) || mode < 0 || mode > 3 || !points_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_fft(ctx->c, group, points_dev, log_n, mode, pick_stream(ctx, stream));
}
int bh_point_distribute_powers_dev(bh_ctx *ctx, int group, void *points_dev, size_t n, const void *g_host, void *stream) {
  if (!ctx || !group_ok(group) || !g_host) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  fr_t g;
  memcpy(&g, g_host, sizeof g);
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_distribute_powers(ctx->c, group, points_dev, n, g, pick_stream(ctx, stream));
}
int bh_point_divide_by_z_on_coset_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !group_ok(group) || !points_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_divide_by_z(group, points_dev, log_n, pick_stream(ctx, stream));
}
int bh_point_mul_assign_dev(bh_ctx *ctx, int group, void *points_dev, const void *scalars_dev, size_t n, void *stream) {
  if (!ctx || !group_ok(group)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_mul_assign(group, points_dev, scalars_dev, n, pick_stream(ctx, stream));
}
int bh_point_sub_assign_dev(bh_ctx *ctx, int group, void *a_dev, const void *b_dev, size_t n, void *stream) {
  if (!ctx || !group_ok(group)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_sub_assign(group, a_dev, b_dev, n, pick_stream(ctx, stream));
}
int bh_fr_powers_dev(bh_ctx *ctx, void *out, size_t n, const void *g_host, const void *scale_host, void *stream) {
  fr_t g, sc;
  memcpy(&g, g_host, sizeof g);
  memcpy(&sc, scale_host, sizeof sc);
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return fr_gen_powers(ctx->c, (fr_t *)out, n, g, sc, pick_stream(ctx, stream));
}
int bh_h_poly_fr_dev_on(bh_ctx *ctx, void *a, void *b, void *c, void *scratch, uint32_t log_n, void *stream) {
  // enqueue only: the caller owns `scratch` (2^log_n Fr; may be null up to 2^11) until the stream has drained
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !a || !b || !c || (log_n > 11 && !scratch)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return h_poly_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, (fr_t *)scratch, log_n, pick_stream(ctx, stream));
}
int bh_h_poly_fr_dev(bh_ctx *ctx, void *a, void *b, void *c, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = ctx->c.pool.acquire(sizeof(fr_t) << log_n);
  if (!scratch) return BH_ERR_HIP;
  int rc = h_poly_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, (fr_t *)scratch, log_n, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  ctx->c.pool.release(scratch);
  return rc;
}
int bh_h_poly_fr(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host, size_t n_evals,
                 void *h_out_host, size_t *h_len) {
  // EvaluationDomain::from_coeffs (domain.rs:47-79): m = next power of two >= len, zero padded
  uint32_t log_n = 0;
  size_t m = 1;
  while (m < n_evals) {
    m *= 2;
    log_n++;
    if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  }
  const size_t bytes = sizeof(fr_t) * m, in_bytes = sizeof(fr_t) * n_evals;
  void *d[3] = {ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes)};
  const void *h[3] = {a_host, b_host, c_host};
  int rc = (d[0] && d[1] && d[2]) ? BH_OK : BH_ERR_HIP;
  for (int i = 0; i < 3 && rc == BH_OK; i++) {
    if (hipMemsetAsync(d[i], 0, bytes, ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
    if (rc == BH_OK && in_bytes &&
        hipMemcpyAsync(d[i], h[i], in_bytes, hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess)
      rc = BH_ERR_HIP;
  }
  if (rc == BH_OK) rc = bh_h_poly_fr_dev(ctx, d[0], d[1], d[2], log_n, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, h_out_host, d[0], sizeof(fr_t) * (m - 1));   // prover.rs:238-239
  if (h_len) *h_len = m - 1;
  for (int i = 0; i < 3; i++) ctx->c.pool.release(d[i]);
  return rc;
}

int bh_h_poly_fr_scalars(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host, size_t n_evals,
                         bh_scalars **h_out) {
  if (!ctx || !h_out || (n_evals && (!a_host || !b_host || !c_host))) return BH_ERR_INVALID_ARG;
  uint32_t log_n = 0;
  size_t m = 1;
  while (m < n_evals) {   // EvaluationDomain::from_coeffs (domain.rs:47-79)
    m *= 2;
    log_n++;
    if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t bytes = sizeof(fr_t) * m, in_bytes = sizeof(fr_t) * n_evals;
  // the three vectors are staged on three streams so that the copies of b and c overlap the first transforms... the
  // h block itself is a dependent chain, so: one caller-private stream (concurrent proofs do not serialise on the
  // context stream)
  void *stv = nullptr;
  int rc = bh_stream_create(ctx, &stv);
  if (rc != BH_OK) return rc;
  hipStream_t st = (hipStream_t)stv;
  void *d[3] = {ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes)};
  void *scratch = log_n > 11 ? ctx->c.pool.acquire(bytes) : nullptr;
  const void *h[3] = {a_host, b_host, c_host};
  rc = (d[0] && d[1] && d[2] && (log_n <= 11 || scratch)) ? BH_OK : BH_ERR_HIP;
  for (int i = 0; i < 3 && rc == BH_OK; i++) {
    if (m > n_evals && hipMemsetAsync((char *)d[i] + in_bytes, 0, bytes - in_bytes, st) != hipSuccess) rc = BH_ERR_HIP;
    if (rc == BH_OK && in_bytes && hipMemcpyAsync(d[i], h[i], in_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
      rc = BH_ERR_HIP;
  }
  if (rc == BH_OK) rc = h_poly_dev(ctx->c, (fr_t *)d[0], (fr_t *)d[1], (fr_t *)d[2], (fr_t *)scratch, log_n, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  (void)bh_stream_destroy(ctx, stv);
  ctx->c.pool.release(d[1]);
  ctx->c.pool.release(d[2]);
  ctx->c.pool.release(scratch);
  if (rc != BH_OK) { ctx->c.pool.release(d[0]); return rc; }
  *h_out = new bh_scalars{ctx, d[0], m - 1, BH_SCALARS_MONT, true};   // a.len() - 1 coefficients, prover.rs:238-239
  return BH_OK;
}

}  // extern "C"
