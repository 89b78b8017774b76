// out[i] = [s_i] in[i] over a vector of affine G1 / G2 records with one scalar per point: what a powers-of-tau
// contributor does to every point of the four vectors (T[i] -> [tau^i] T[i], ...), by the split-scalar ladder of
// glv.cuh - 128 joint steps over (k mod lambda, k div lambda) instead of the 255 of point_fft.hip's xyzz_mul_fr.
// One lane per point, grid-stride; the scalar is an element of a vector (Montgomery or canonical), and the powers
// c g^i of bh_bases_scale_powers are such a vector, built in front by launch_gen_powers (fft.hip).  Affine
// out, one inversion per lane as everywhere; `out` may alias `in` (a lane reads its record before it writes it).
#include "common.hpp"
#include "fft.hpp"
#include "glv.cuh"
#include "point_ops.hpp"

namespace bh {
namespace {

// one wavefront per block: the G1 kernel is sized for one wave per SIMD, and 2^16 points are then one wave on every SIMD
constexpr u32 PM_THREADS = 64;
constexpr u64 PM_MAX_BLOCKS = 1u << 20;   // grid-stride beyond 2^26 lanes

template <class F>
__global__ __launch_bounds__(PM_THREADS) void pm_each_kernel(const Affine<F> *in, Affine<F> *out, u64 n, const fr_t *scalars,
                                                             int mont) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const fr_t v = scalars[i];
    fr_t k;
    if (mont) {
      fe_from_mont(k, v);
    } else {
      k = v;
      glv_reduce_canonical(k);
    }
    const Affine<F> a = in[i];
    XYZZ<F> x;
    xyzz_mul_glv(x, a, k);
    Affine<F> r;
    xyzz_to_affine(r, x);
    out[i] = r;
  }
}

template <class F>
int pm_launch(const void *in, void *out, u64 n, const void *scalars, int mont, hipStream_t st) {
  const u64 b = (n + PM_THREADS - 1) / PM_THREADS;
  hipLaunchKernelGGL(pm_each_kernel<F>, dim3((u32)(b < PM_MAX_BLOCKS ? b : PM_MAX_BLOCKS)), dim3(PM_THREADS), 0, st,
                     (const Affine<F> *)in, (Affine<F> *)out, n, (const fr_t *)scalars, mont);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
}  // namespace

// enqueues out[i] = [scalars[i]] in[i]; n > 0
int point_mul_each(int group, const void *in, void *out, u64 n, const void *scalars, int fmt, hipStream_t st) {
  const int mont = fmt == BH_SCALARS_MONT;
  return group == BH_G1 ? pm_launch<FpOps>(in, out, n, scalars, mont, st) : pm_launch<Fp2Ops>(in, out, n, scalars, mont, st);
}
// out[i] = [c g^i] in[i] (c, g Montgomery): the powers in a pool vector, then one multiplication per point; waits for
// the stream.  Both groups take this multiplier: it is faster than the ladder at every size measured.
int point_mul_powers(Context &c, int group, const void *in, void *out, u64 n, const fr_t &cc, const fr_t &g, hipStream_t st) {
  fr_t *pw = (fr_t *)c.pool.acquire(n * sizeof(fr_t));
  if (!pw) return BH_ERR_HIP;
  int rc = launch_gen_powers(pw, n, g, cc, 0, st);
  if (rc == BH_OK) rc = point_mul_each(group, in, out, n, pw, BH_SCALARS_MONT, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  c.pool.release(pw);
  return rc;
}

}  // namespace bh
