// Test hooks of the powers-of-tau check (include/bellman_hip_test.h): the coefficient expander of ptau_rlc.cuh on the host
// and on the device, and the eight sums of a transcript - the text the product's ceremony.hip compiles, run on its own
// (tests/test_ptau_verify_cpu.py, tests/test_gpu_ptau_verify.py).
#include "../../include/bellman_hip_test.h"
#include "ptau_rlc.cuh"

using namespace bh;

extern "C" {

void bh_test_ptau_rlc_host(const void *seed32, uint32_t v, size_t count, void *out_host) {
  ptau_rlc_host(seed32, v, count, out_host);
}

int bh_test_ptau_rlc_dev(bh_ctx *ctx, const void *seed32, uint32_t v, size_t count, void *out_host) {
  if (!ctx || !seed32 || (count && !out_host)) return BH_ERR_INVALID_ARG;
  if (!count) return BH_OK;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  // one guard scalar behind the last coefficient: an odd count must not write the second half of its last block
  u32 *d = (u32 *)c.pool.acquire((count + 1) * 32);
  if (!d) return BH_ERR_HIP;
  u32 guard[8];
  int rc = BH_OK;
  if (hipMemsetAsync(d, 0xa5, (count + 1) * 32, c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (!rc) rc = ptau_rlc_expand(c.stream, seed32, v, count, d);
  if (!rc && (hipMemcpyAsync(out_host, d, count * 32, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
              hipMemcpyAsync(guard, d + 8 * count, 32, hipMemcpyDeviceToHost, c.stream) != hipSuccess))
    rc = BH_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess && !rc) rc = BH_ERR_HIP;
  c.pool.release(d);
  if (!rc)
    for (int i = 0; i < 8; i++)
      if (guard[i] != 0xa5a5a5a5u) rc = BH_ERR_INVALID_ARG;   // the expander wrote past `count` coefficients
  return rc;
}

int bh_test_ptau_sums(bh_ctx *ctx, const bh_powers_of_tau *t, const void *seed32, void *sums_out, int *rcs_out) {
  if (!ctx || !t || !seed32 || !sums_out || !rcs_out) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const bh_bases *vec[4] = {t->tau_g1, t->tau_g2, t->alpha_tau_g1, t->beta_tau_g1};
  void *st = nullptr;
  int rc = bh_stream_create(ctx, &st);
  if (rc) return rc;
  rc = ptau_sums(ctx, vec, seed32, (hipStream_t)st, (unsigned char(*)[192])sums_out, rcs_out);
  (void)hipStreamSynchronize((hipStream_t)st);
  bh_stream_destroy(ctx, st);
  return rc;
}

}  // extern "C"
