// The verifier's launch functions that other units call: the definitions are in pairing_kernels.cuh, which one unit per
// library compiles (pairing.hip in the product, test_pairing_hooks.hip in the test library).  Used by ceremony.hip and by
// test_hooks.hip (bh_test_pairing).  The launch functions only the verifier itself runs are static in pairing_kernels.cuh.
#pragma once
#include "common.hpp"
#include "fp12.cuh"

namespace bh {
int launch_g2_lines(hipStream_t st, const void *q_dev, size_t stride_bytes, int negate, line_t *lines, u32 *flags, size_t n);
int launch_miller(hipStream_t st, const Affine<FpOps> *p, const line_t *lines, const u32 *qflags, fp12_t *f, size_t n,
                  const line_t *lines1 = nullptr, const u32 *qflags1 = nullptr, size_t n1 = 0);
int launch_fold(hipStream_t st, fp12_t *f, size_t m);
int launch_fold_rows(hipStream_t st, fp12_t *f, size_t m);
int launch_final_exp(hipStream_t st, const fp12_t *f, size_t n, fp12_t *out, u32 *is_one, fp12_t *ws);
}  // namespace bh
