// Test hooks of the split-scalar point multiplier (include/bellman_hip_test.h): glv_split on the host, and the joint
// ladder xyzz_mul_glv over arbitrary 128-bit pairs on the host and in a kernel of one lane per point - the text the
// product's point_mul.hip compiles, the split and the ladder apart (tests/test_glv_cpu.py, tests/test_gpu_point_mul_each.py).
#include <string.h>

#include "../../include/bellman_hip_test.h"
#include "common.hpp"
#include "glv.cuh"

namespace bh {
namespace {

template <class F>
__global__ __launch_bounds__(64) void glv_ladder_kernel(const Affine<F> *p, const glv_half *k1, const glv_half *k2, u64 n,
                                                        Affine<F> *out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> a = p[i];
  XYZZ<F> x;
  xyzz_mul_glv(x, a, k1[i], k2[i]);
  Affine<F> r;
  xyzz_to_affine(r, x);
  out[i] = r;
}

template <class F>
void ladder_host(const char *points, const char *k1, const char *k2, size_t n, char *out) {
  for (size_t i = 0; i < n; i++) {   // host buffers carry no alignment promise
    Affine<F> a, r;
    glv_half h1, h2;
    memcpy(&a, points + i * sizeof a, sizeof a);
    memcpy(&h1, k1 + i * 16, 16);
    memcpy(&h2, k2 + i * 16, 16);
    XYZZ<F> x;
    xyzz_mul_glv(x, a, h1, h2);
    xyzz_to_affine(r, x);
    memcpy(out + i * sizeof r, &r, sizeof r);
  }
}

}  // namespace
}  // namespace bh

using namespace bh;

extern "C" {

void bh_test_glv_split_host(const void *k, void *k1, void *k2, size_t n) {
  for (size_t i = 0; i < n; i++) {
    fr_t s;
    glv_half h1, h2;
    memcpy(&s, (const char *)k + i * 32, 32);
    glv_split(s, h1, h2);
    memcpy((char *)k1 + i * 16, &h1, 16);
    memcpy((char *)k2 + i * 16, &h2, 16);
  }
}

int bh_test_glv_ladder_host(int group, const void *points, const void *k1, const void *k2, size_t n, void *out) {
  if ((group != BH_G1 && group != BH_G2) || (n && (!points || !k1 || !k2 || !out))) return BH_ERR_INVALID_ARG;
  if (group == BH_G1) ladder_host<FpOps>((const char *)points, (const char *)k1, (const char *)k2, n, (char *)out);
  else ladder_host<Fp2Ops>((const char *)points, (const char *)k1, (const char *)k2, n, (char *)out);
  return BH_OK;
}

int bh_test_glv_ladder_dev(bh_ctx *ctx, int group, const void *points, const void *k1, const void *k2, size_t n, void *out) {
  if (!ctx || (group != BH_G1 && group != BH_G2) || n > (1u << 20) || (n && (!points || !k1 || !k2 || !out))) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  const size_t rec = group == BH_G1 ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  // points | out | k1 | k2, every part a multiple of 16 bytes
  char *d = (char *)c.pool.acquire(n * (2 * rec + 32));
  if (!d) return BH_ERR_HIP;
  char *d_out = d + n * rec, *d_k1 = d_out + n * rec, *d_k2 = d_k1 + n * 16;
  hipStream_t st = c.stream;
  int rc = BH_OK;
  if (hipMemcpyAsync(d, points, n * rec, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_k1, k1, n * 16, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_k2, k2, n * 16, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = BH_ERR_HIP;
  if (!rc) {
    const dim3 grid((u32)((n + 63) / 64));
    if (group == BH_G1)
      hipLaunchKernelGGL(glv_ladder_kernel<FpOps>, grid, dim3(64), 0, st, (const Affine<FpOps> *)d, (const glv_half *)d_k1,
                         (const glv_half *)d_k2, (u64)n, (Affine<FpOps> *)d_out);
    else
      hipLaunchKernelGGL(glv_ladder_kernel<Fp2Ops>, grid, dim3(64), 0, st, (const Affine<Fp2Ops> *)d, (const glv_half *)d_k1,
                         (const glv_half *)d_k2, (u64)n, (Affine<Fp2Ops> *)d_out);
    if (hipGetLastError() != hipSuccess) rc = BH_ERR_HIP;
  }
  if (!rc && hipMemcpyAsync(out, d_out, n * rec, hipMemcpyDeviceToHost, st) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
  c.pool.release(d);
  return rc;
}

}  // extern "C"
