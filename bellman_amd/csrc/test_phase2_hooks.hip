// Test hooks of the ceremony-step check (include/bellman_hip_test.h): the four sums of a step - the text the product's
// ceremony.hip compiles, run on its own - and the comparison kernel's per-record predicate built for the host
// (tests/test_phase2_cpu.py, tests/test_gpu_phase2.py).
#include "../../include/bellman_hip_test.h"
#include "bases_compare.cuh"
#include "phase2_sums.cuh"

using namespace bh;

extern "C" {

int bh_test_phase2_sums(bh_ctx *ctx, const bh_params *before, const bh_params *after, const void *seed32, void *sums_out,
                        int *rcs_out) {
  if (!ctx || !before || !after || !seed32 || !sums_out || !rcs_out) return BH_ERR_INVALID_ARG;
  const bh_bases *q[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < 4; k++) {
    const int rc = bh_groth16_params_query(k & 1 ? after : before, k / 2, &q[k], nullptr);
    if (rc) return rc;
  }
  if (bh_bases_len(q[0]) != bh_bases_len(q[1]) || bh_bases_len(q[2]) != bh_bases_len(q[3])) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  void *st = nullptr;
  int rc = bh_stream_create(ctx, &st);
  if (rc) return rc;
  rc = phase2_sums(ctx, q, seed32, (hipStream_t)st, (unsigned char(*)[96])sums_out, rcs_out);
  (void)hipStreamSynchronize((hipStream_t)st);
  bh_stream_destroy(ctx, st);
  return rc;
}

int bh_test_records_differ_host(int group, const void *a, const void *b, size_t n, unsigned char *out) {
  if ((group != BH_G1 && group != BH_G2) || (n && (!a || !b || !out)) || (((uintptr_t)a | (uintptr_t)b) & 15))
    return BH_ERR_INVALID_ARG;
  const uint4 *va = (const uint4 *)a, *vb = (const uint4 *)b;
  for (size_t i = 0; i < n; i++)
    out[i] = group == BH_G1 ? records_differ<6>(va + 6 * i, vb + 6 * i) : records_differ<12>(va + 12 * i, vb + 12 * i);
  return BH_OK;
}

void bh_test_compare_shape(uint32_t out2[2]) {
  out2[0] = COMPARE_THREADS;
  out2[1] = COMPARE_MAX_BLOCKS;
}

}  // extern "C"
