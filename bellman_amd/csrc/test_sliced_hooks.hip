// libbellman_hip_test.so: the mixed addition of the G1 bucket accumulation (ec.cuh xyzz_madd_sliced: every value cut into
// 30-bit limbs once, products over the limbs) next to xyzz_madd on raw projective operands the caller chooses, raw results
// back (bh_test_g1_madd_sliced_dev / _host of include/bellman_hip_test.h; tests/test_gpu_madd_sliced.py).  The same function
// runs in the kernel and in the host loop.
#include "../../include/bellman_hip_test.h"
#include "handles.hpp"
#include "msm_workers.cuh"

namespace bh {
namespace slicedops {

// flag word: bit 0 xyzz_madd returned true, bit 1 xyzz_madd_sliced did, bit 4 the base was the identity (skipped, as the
// accumulation does: both results = a).  The sliced addition is the form msm_accumulate_kernel<FpOps, false> runs: products inline.
BH_HD u32 one_case(XYZZ<FpOps> &ref, XYZZ<FpOps> &chk, const XYZZ<FpOps> &a, const Affine<FpOps> &q) {
  ref = a;
  chk = a;
  if (aff_is_identity(q)) return 16u;
  return (xyzz_madd(ref, q) ? 1u : 0u) | (xyzz_madd_sliced<FpOps, true>(chk, q) ? 2u : 0u);
}

__global__ __launch_bounds__(128) void madd_sliced_kernel(XYZZ<FpOps> *r, u32 *flags, const XYZZ<FpOps> *a, const Affine<FpOps> *q, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  XYZZ<FpOps> pa, ref, chk;
  Affine<FpOps> pq;
  load_xyzz<FpOps>(pa, a + i);
  load_affine<FpOps>(pq, q + i);
  flags[i] = one_case(ref, chk, pa, pq);
  store_xyzz<FpOps>(r + i, ref);
  store_xyzz<FpOps>(r + n + i, chk);
}

}  // namespace slicedops
}  // namespace bh

using namespace bh;
extern "C" {
int bh_test_g1_madd_sliced_dev(bh_ctx *ctx, void *r_dev, uint32_t *flags_dev, const void *a_dev, const void *q_dev, size_t n) {
  if (!ctx || !r_dev || !flags_dev || !a_dev || !q_dev || n > (1u << 20)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = ctx->c.stream;
  slicedops::madd_sliced_kernel<<<(unsigned)((n + 127) / 128), 128, 0, st>>>((XYZZ<FpOps> *)r_dev, flags_dev, (const XYZZ<FpOps> *)a_dev,
                                                                             (const Affine<FpOps> *)q_dev, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  BH_HIP_CHECK(hipStreamSynchronize(st));
  return BH_OK;
}
int bh_test_g1_madd_sliced_host(void *r, uint32_t *flags, const void *a, const void *q, size_t n) {
  if (!r || !flags || !a || !q) return BH_ERR_INVALID_ARG;
  XYZZ<FpOps> *out = (XYZZ<FpOps> *)r;
  for (size_t i = 0; i < n; i++)
    flags[i] = slicedops::one_case(out[i], out[n + i], ((const XYZZ<FpOps> *)a)[i], ((const Affine<FpOps> *)q)[i]);
  return BH_OK;
}
}  // extern "C"
