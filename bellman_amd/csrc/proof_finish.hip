// k proofs from k sets of multiexp sums on the device (proof_finish.cuh; prover.rs:320-360): stage 1 multiplies, one lane
// per (proof, product), into an XYZZ workspace; stage 2 adds, inverts and writes the 384-byte records, one lane per proof
// element.  G1 and G2 multiply in kernels of their own: the G2 ladder spills registers and must not set
// the G1 kernel's budget.  The work is latency-bound at the batch sizes it serves (k = 256: 32 wavefronts of G1 lanes),
// so blocks are one wavefront, as in point_mul.hip.
#include <string.h>

#include "common.hpp"
#include "proof_finish.cuh"

namespace bh {
namespace {

constexpr u32 PF_THREADS = 64;

// lane i: product i % 8 of proof i / 8 (G1), or proof i's one product (G2)
template <class F>
__global__ __launch_bounds__(PF_THREADS) void finish_mul_kernel(const FinishKey key, const FinishSums *sums, const fr_t *r, const fr_t *s,
                                                                u64 lanes, XYZZ<F> *out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;
  XYZZ<F> x;
  if constexpr (std::is_same<F, FpOps>::value) {
    const u64 j = i / PF_G1_PRODUCTS;
    finish_mul_g1(x, key, sums[j], r[j], s[j], (int)(i % PF_G1_PRODUCTS));
  } else {
    finish_mul_g2(x, key, s[i]);
  }
  out[i] = x;
}

// blockIdx.y: the proof element, so that a block runs one group's code
__global__ __launch_bounds__(PF_THREADS) void finish_sum_kernel(const FinishKey key, const FinishSums *sums, const XYZZ<FpOps> *g1,
                                                                const XYZZ<Fp2Ops> *g2, u64 k, FinishProof *out) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  if (blockIdx.y == PF_A) {
    pf_g1 a;
    finish_sum_a(a, key, sums[j], g1 + j * PF_G1_PRODUCTS);
    out[j].a = a;
  } else if (blockIdx.y == PF_B) {
    pf_g2 b;
    finish_sum_b(b, key, sums[j], g2[j]);
    out[j].b = b;
  } else {
    pf_g1 c;
    finish_sum_c(c, sums[j], g1 + j * PF_G1_PRODUCTS);
    out[j].c = c;
  }
}

}  // namespace

// enqueues both stages on st; ws holds k * PROOF_FINISH_WS_BYTES bytes
constexpr size_t PROOF_FINISH_WS_BYTES = PF_G1_PRODUCTS * sizeof(XYZZ<FpOps>) + sizeof(XYZZ<Fp2Ops>);
static int proof_finish_launch(const FinishKey &key, const void *sums, const void *r, const void *s, u64 k, void *ws, void *proofs,
                               hipStream_t st) {
  XYZZ<FpOps> *g1 = (XYZZ<FpOps> *)ws;
  XYZZ<Fp2Ops> *g2 = (XYZZ<Fp2Ops> *)(g1 + k * PF_G1_PRODUCTS);
  const u64 lanes1 = k * PF_G1_PRODUCTS;
  const dim3 block(PF_THREADS);
  hipLaunchKernelGGL(finish_mul_kernel<FpOps>, dim3((u32)((lanes1 + PF_THREADS - 1) / PF_THREADS)), block, 0, st, key,
                     (const FinishSums *)sums, (const fr_t *)r, (const fr_t *)s, lanes1, g1);
  BH_HIP_CHECK(hipGetLastError());
  const u32 blocks = (u32)((k + PF_THREADS - 1) / PF_THREADS);
  hipLaunchKernelGGL(finish_mul_kernel<Fp2Ops>, dim3(blocks), block, 0, st, key, (const FinishSums *)sums, (const fr_t *)r,
                     (const fr_t *)s, k, g2);
  BH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(finish_sum_kernel, dim3(blocks, PF_ELEMENTS), block, 0, st, key, (const FinishSums *)sums,
                     (const XYZZ<FpOps> *)g1, (const XYZZ<Fp2Ops> *)g2, k, (FinishProof *)proofs);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // namespace bh

using namespace bh;

extern "C" int bh_proof_finish_dev(bh_ctx *ctx, const void *vk5, const void *sums_dev, const void *r_dev, const void *s_dev, size_t k,
                                   void *proofs_dev, void *stream) {
  if (!ctx || !vk5 || k > (size_t(1) << 24)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!sums_dev || !r_dev || !s_dev || !proofs_dev) return BH_ERR_INVALID_ARG;
  FinishKey key;
  memcpy(&key, vk5, sizeof key);
  if (aff_is_identity(key.delta_g1) || aff_is_identity(key.delta_g2)) return BH_ERR_UNEXPECTED_IDENTITY;   // prover.rs:320-324
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  hipStream_t st = stream ? (hipStream_t)stream : c.stream;
  void *ws = c.pool.acquire(k * PROOF_FINISH_WS_BYTES);
  if (!ws) return BH_ERR_HIP;
  int rc = proof_finish_launch(key, sums_dev, r_dev, s_dev, k, ws, proofs_dev, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;   // the workspace is free again from here
  c.pool.release(ws);
  return rc;
}
