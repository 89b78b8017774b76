// The final exponentiation of fp12.cuh (f12_final_exp) as a chain of small kernels over n independent values, with the
// intermediate Fp12 values in device memory.  As one inlined kernel the whole chain needed 25 KB of scratch per lane
// (14 800 spilled VGPRs), which the runtime must provide per queue for every launch; each step below keeps at most
// three Fp12 values live, and the exponentiations by x alternate runs of cyclotomic squarings
// (no scratch) with products.  Included by pairing.hip (the verifier) and test_hooks.hip (the pairing test hook).
#pragma once
#include <hip/hip_runtime.h>

#include "fp12.cuh"

namespace bh {

// out = a * op(b); op: 0 b, 1 conj(b), 2 b^p, 3 b^(p^2)
__global__ __launch_bounds__(64) static void fe_mul_op_kernel(const fp12_t *a, const fp12_t *b, int op, fp12_t *out, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t x = b[i], y;
  if (op == 1) f12_conj(y, x);
  else if (op == 2) f12_frob1(y, x);
  else if (op == 3) f12_frob2(y, x);
  else y = x;
  x = a[i];
  f12_mul(x, x, y);
  out[i] = x;
}
// m = f^((p^6 - 1)(p^2 + 1))
__global__ __launch_bounds__(64) static void fe_easy_kernel(const fp12_t *f, fp12_t *m, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t a = f[i], t;
  f12_inv(t, a);
  f12_conj(a, a);
  f12_mul(a, a, t);
  m[i] = a;
}
// out = in^(2^k) (k cyclotomic squarings; in-place allowed)
__global__ __launch_bounds__(64) static void fe_cyc_sqr_kernel(const fp12_t *in, fp12_t *out, int k, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t a = in[i];
#pragma unroll 1
  for (int j = 0; j < k; j++) f12_cyc_sqr(a, a);
  out[i] = a;
}
__global__ __launch_bounds__(64) static void fe_conj_kernel(fp12_t *a, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t x = a[i];
  f12_conj(x, x);
  a[i] = x;
}
// r = canonical(r); is_one[i] = (r == 1)
__global__ __launch_bounds__(64) static void fe_finish_kernel(fp12_t *r, u32 *is_one, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t a = r[i];
  f12_canon(a);
  r[i] = a;
  if (is_one) is_one[i] = f12_is_one(a) ? 1u : 0u;
}

// out = in^x (in cyclotomic, out != in): square-and-multiply over |x| in runs of squarings, then the conjugate (x < 0)
static bool exp_x_chain(hipStream_t st, const fp12_t *in, fp12_t *out, u32 n) {
  const dim3 g((n + 63) / 64), blk(64);
  if (hipMemcpyAsync(out, in, n * sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
  int run = 0;
  for (int i = 62; i >= 0; i--) {
    run++;
    if ((BLS_X_ABS >> i) & 1) {
      hipLaunchKernelGGL(fe_cyc_sqr_kernel, g, blk, 0, st, out, out, run, n);
      hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, out, in, 0, out, n);
      run = 0;
    }
  }
  if (run) hipLaunchKernelGGL(fe_cyc_sqr_kernel, g, blk, 0, st, out, out, run, n);
  hipLaunchKernelGGL(fe_conj_kernel, g, blk, 0, st, out, n);
  return true;
}

// out[i] = f[i]^(3 (p^12 - 1) / q), canonical (the chain of f12_final_exp); ws = 4 n Fp12 of device workspace; returns
// false when a launch failed.  out may alias f.
static bool final_exp_chain(hipStream_t st, const fp12_t *f, fp12_t *out, u32 *is_one, fp12_t *ws, u32 n) {
  if (!n) return true;
  fp12_t *m = ws, *a = ws + n, *b = ws + 2 * n, *t = ws + 3 * n;
  const dim3 g((n + 63) / 64), blk(64);
  (void)hipGetLastError();   // a handled error of an earlier call on this thread is not ours
  hipLaunchKernelGGL(fe_easy_kernel, g, blk, 0, st, f, t, n);           // t = f^(p^6 - 1)
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, t, t, 3, m, n);   // m = t * t^(p^2)
  if (!exp_x_chain(st, m, a, n)) return false;
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, a, m, 1, a, n);   // a = m^(x - 1)
  if (!exp_x_chain(st, a, t, n)) return false;
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, t, a, 1, a, n);   // a = m^((x - 1)^2)
  if (!exp_x_chain(st, a, b, n)) return false;
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, b, a, 2, b, n);   // b = a^(x + p)
  if (!exp_x_chain(st, b, t, n)) return false;
  if (!exp_x_chain(st, t, a, n)) return false;
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, a, b, 3, a, n);
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, a, b, 1, a, n);   // a = b^(x^2 + p^2 - 1)
  hipLaunchKernelGGL(fe_cyc_sqr_kernel, g, blk, 0, st, m, t, 1, n);
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, t, m, 0, t, n);   // t = m^3
  hipLaunchKernelGGL(fe_mul_op_kernel, g, blk, 0, st, a, t, 0, out, n);
  hipLaunchKernelGGL(fe_finish_kernel, g, blk, 0, st, out, is_one, n);
  return hipGetLastError() == hipSuccess;
}

}  // namespace bh
