// EvaluationDomain<Fr, Point<G>> (src/domain.rs:192-229 with the generic methods of :21-190) for G1 and G2 on gfx950:
// the transforms of a vector of group elements by Fr twiddles - what turns a powers-of-tau transcript [tau^i]G into the
// Lagrange-basis points [L_j(tau)]G (the group-side twin of generator.rs:299-300).
//
//   fft / ifft / coset_fft / icoset_fft (:81-125)  ->  point_fft()
//     radix-2 DIT after a bit-reversal permutation (serial_fft, :272-314): one launch per stage, one lane per butterfly,
//     points in XYZZ form in a pool workspace between stages, affine (one inversion per lane) once at the end.  Group
//     elements are unique, so any evaluation order of the same linear map gives the reference's records: coset_fft
//     multiplies by 7^i while loading, ifft / icoset_fft multiply by 1/n resp. 7^-i / n while storing.
//   distribute_powers (:101-113), divide_by_z_on_coset (:139-151), mul_assign (:154-170), sub_assign (:173-189)
//     -> the element-wise kernels at the bottom.
//
// A butterfly's work is one variable-base scalar multiplication [w]b by an Fr twiddle (skipped for w = 1) and two
// additions: a + [w]b, a - [w]b.  The multiplication is a fixed MSB-first double-and-add ladder over the 255 bits of the
// canonical twiddle on XYZZ points (ec.cuh: xyzz_dbl 9 Fp products, xyzz_add 14; G2 Karatsuba: 24 / 40).  Butterflies
// are numbered twiddle-major (lane t: j = t >> log(n/2m), block = t & (n/2m - 1)), so in every stage with n/2m >= 64
// all lanes of a wavefront share one twiddle and the ladder's branches are uniform; only the last six stages mix
// twiddles within a wavefront.  Identity, equal and opposite operands (zero padding, constant inputs) take
// xyzz_add's own branches.
#include "common.hpp"
#include "fft.hpp"   // the Fr power tables and domain constants shared with the scalar transforms
#include "point_ops.hpp"

namespace bh {
namespace {

constexpr u32 PF_THREADS = 128;
constexpr u64 PF_MAX_BLOCKS = 1u << 20;   // grid-stride beyond 2^27 lanes

// where a kernel's per-element scalar comes from
enum : int { PF_NONE = 0, PF_CONST = 1, PF_VEC = 2 };
struct PfScalar {
  const fr_t *vec;   // PF_VEC: Montgomery Fr per element
  fr_t k;            // PF_CONST: canonical Fr
  int kind;
};

__device__ __forceinline__ bool pf_scalar(const PfScalar &s, u64 i, fr_t &k) {
  if (s.kind == PF_CONST) {
    k = s.k;
  } else if (s.kind == PF_VEC) {
    fr_t m = s.vec[i];
    fe_from_mont(k, m);
  } else {
    return false;
  }
  return true;
}

// r = [k] p for a canonical k < 2^255 (Fr): MSB-first double-and-add, the same 255 steps in every lane.  Leading zero
// bits double the identity (ec.cuh returns at once); the first set bit copies p.  r may alias p only through the
// temporary below.
template <class F>
__device__ __forceinline__ void xyzz_mul_fr(XYZZ<F> &r, const XYZZ<F> &p, const fr_t &k) {
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  for (int i = 254; i >= 0; i--) {
    xyzz_dbl(acc, acc);
    if ((k.l[i >> 5] >> (i & 31)) & 1u) xyzz_add(acc, acc, p);
  }
  r = acc;
}

template <class F>
__device__ __forceinline__ void xyzz_neg(XYZZ<F> &p) {
  F::neg(p.y, p.y);
}

__device__ __forceinline__ u64 bitrev(u64 i, u32 log_n) { return log_n ? __brevll(i) >> (64 - log_n) : 0; }

// ws[bitrev(i)] = [s_i] in[i]  (coset_fft's 7^i while loading; otherwise a copy into XYZZ)
template <class F>
__global__ __launch_bounds__(PF_THREADS) void pf_load_kernel(const Affine<F> *in, XYZZ<F> *ws, u64 n, u32 log_n,
                                                             PfScalar s) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const Affine<F> a = in[i];
    XYZZ<F> x;
    xyzz_from_affine(x, a);
    fr_t k;
    if (pf_scalar(s, i, k)) xyzz_mul_fr(x, x, k);
    ws[bitrev(i, log_n)] = x;
  }
}

// one DIT stage of half-size m = 2^s (serial_fft's inner loops, :296-311): for each butterfly (block, j)
//   t = [w_m^j] a[k + j + m];  a[k + j + m] = a[k + j] - t;  a[k + j] += t      (w_m = omega^(n / 2m); tw[e] = omega^e)
template <class F>
__global__ __launch_bounds__(PF_THREADS) void pf_stage_kernel(XYZZ<F> *ws, const fr_t *tw, u32 log_n, u32 s) {
  const u64 half = (u64)1 << (log_n - 1);
  const u32 lnb = log_n - 1 - s;   // log2 of the number of blocks, n / 2m
  const u64 nb_mask = ((u64)1 << lnb) - 1;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < half; t += (u64)gridDim.x * blockDim.x) {
    const u64 j = t >> lnb, blk = t & nb_mask;
    const u64 i0 = (blk << (s + 1)) + j, i1 = i0 + ((u64)1 << s);
    XYZZ<F> b = ws[i1];
    if (j) {   // w = 1 for j = 0: no multiplication
      fr_t w, wm = tw[j << lnb];
      fe_from_mont(w, wm);
      xyzz_mul_fr(b, b, w);
    }
    const XYZZ<F> a = ws[i0];
    XYZZ<F> r;
    xyzz_add(r, a, b);
    ws[i0] = r;
    xyzz_neg(b);
    xyzz_add(r, a, b);
    ws[i1] = r;
  }
}

// out[i] = affine([s_i] ws[i])  (ifft's 1/n, icoset_fft's 7^-i / n)
template <class F>
__global__ __launch_bounds__(PF_THREADS) void pf_store_kernel(const XYZZ<F> *ws, Affine<F> *out, u64 n, PfScalar s) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    XYZZ<F> x = ws[i];
    fr_t k;
    if (pf_scalar(s, i, k)) xyzz_mul_fr(x, x, k);
    Affine<F> a;
    xyzz_to_affine(a, x);
    out[i] = a;
  }
}

// pts[i] = [s_i] pts[i] in place: distribute_powers, divide_by_z_on_coset, mul_assign
template <class F>
__global__ __launch_bounds__(PF_THREADS) void pf_scale_kernel(Affine<F> *pts, u64 n, PfScalar s) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const Affine<F> a = pts[i];
    XYZZ<F> x;
    xyzz_from_affine(x, a);
    fr_t k;
    if (pf_scalar(s, i, k)) xyzz_mul_fr(x, x, k);
    Affine<F> r;
    xyzz_to_affine(r, x);
    pts[i] = r;
  }
}

// a[i] = a[i] - b[i]: sub_assign
template <class F>
__global__ __launch_bounds__(PF_THREADS) void pf_sub_kernel(Affine<F> *a, const Affine<F> *b, u64 n) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    Affine<F> q = b[i];
    if (aff_is_identity(q)) continue;
    const Affine<F> p = a[i];
    XYZZ<F> x;
    xyzz_from_affine(x, p);
    F::neg(q.y, q.y);
    xyzz_madd(x, q);
    Affine<F> r;
    xyzz_to_affine(r, x);
    a[i] = r;
  }
}

u32 pf_blocks(u64 work) {
  const u64 b = (work + PF_THREADS - 1) / PF_THREADS;
  return (u32)(b < PF_MAX_BLOCKS ? (b ? b : 1) : PF_MAX_BLOCKS);
}
PfScalar pf_none() {
  PfScalar s{};
  return s;
}
PfScalar pf_const(const fr_t &mont) {
  PfScalar s = pf_none();
  fe_from_mont(s.k, mont);
  s.kind = PF_CONST;
  return s;
}
PfScalar pf_vec(const fr_t *v) {
  PfScalar s = pf_none();
  s.vec = v;
  s.kind = PF_VEC;
  return s;
}
fr_t fr_one_host() {
  fr_t one;
  fe_one(one);
  return one;
}
fr_t fr_inv_host(const fr_t &a) {
  fr_t r;
  fe_inv(r, a);
  return r;
}

// Enqueues the transform; ws (n XYZZ), tw (n/2 Fr, n > 1) and pw (n Fr, coset modes) are the caller's workspace.
template <class F>
int point_fft_enqueue(Affine<F> *pts, XYZZ<F> *ws, fr_t *tw, fr_t *pw, uint32_t log_n, int mode, hipStream_t st) {
  const u64 n = (u64)1 << log_n;
  const bool inverse = mode == BH_IFFT || mode == BH_ICOSET_FFT;
  const fr_t one = fr_one_host(), g = fr_from_u64_host(7);   // Fr::MULTIPLICATIVE_GENERATOR
  if (n > 1) {
    fr_t omega = fr_domain_omega_host(log_n);
    if (inverse) omega = fr_inv_host(omega);
    int rc = launch_gen_powers(tw, n / 2, omega, one, 0, st);
    if (rc) return rc;
  }
  PfScalar load = pf_none();
  if (mode == BH_COSET_FFT) {
    int rc = launch_gen_powers(pw, n, g, one, 0, st);
    if (rc) return rc;
    load = pf_vec(pw);
  }
  hipLaunchKernelGGL(pf_load_kernel<F>, dim3(pf_blocks(n)), dim3(PF_THREADS), 0, st, (const Affine<F> *)pts, ws, n, log_n,
                     load);
  BH_HIP_CHECK(hipGetLastError());
  for (u32 s = 0; s < log_n; s++) {
    hipLaunchKernelGGL(pf_stage_kernel<F>, dim3(pf_blocks(n / 2)), dim3(PF_THREADS), 0, st, ws, (const fr_t *)tw, log_n, s);
    BH_HIP_CHECK(hipGetLastError());
  }
  PfScalar store = pf_none();
  if (inverse) {
    const fr_t minv = fr_inv_host(fr_from_u64_host(n));
    if (mode == BH_IFFT) {
      store = pf_const(minv);
    } else {   // icoset_fft: 1/n folded into the powers of 7^-1
      int rc = launch_gen_powers(pw, n, fr_inv_host(g), minv, 0, st);
      if (rc) return rc;
      store = pf_vec(pw);
    }
  }
  hipLaunchKernelGGL(pf_store_kernel<F>, dim3(pf_blocks(n)), dim3(PF_THREADS), 0, st, (const XYZZ<F> *)ws, pts, n, store);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

template <class F>
int point_fft_t(Context &c, void *pts, uint32_t log_n, int mode, hipStream_t st) {
  const u64 n = (u64)1 << log_n;
  const bool coset = mode == BH_COSET_FFT || mode == BH_ICOSET_FFT;
  void *ws = c.pool.acquire(n * sizeof(XYZZ<F>));
  void *tw = n > 1 ? c.pool.acquire(n / 2 * sizeof(fr_t)) : nullptr;
  void *pw = coset ? c.pool.acquire(n * sizeof(fr_t)) : nullptr;
  int rc = (ws && (n == 1 || tw) && (!coset || pw)) ? BH_OK : BH_ERR_HIP;
  if (rc == BH_OK) rc = point_fft_enqueue<F>((Affine<F> *)pts, (XYZZ<F> *)ws, (fr_t *)tw, (fr_t *)pw, log_n, mode, st);
  // the workspace may be recycled by another stream: fence before returning it
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  for (void *p : {ws, tw, pw})
    if (p) c.pool.release(p);
  return rc;
}

template <class F>
int point_scale_t(Affine<F> *pts, u64 n, PfScalar s, hipStream_t st) {
  hipLaunchKernelGGL(pf_scale_kernel<F>, dim3(pf_blocks(n)), dim3(PF_THREADS), 0, st, pts, n, s);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
int point_scale(int group, void *pts, u64 n, PfScalar s, hipStream_t st) {
  return group == BH_G1 ? point_scale_t<FpOps>((Affine<FpOps> *)pts, n, s, st)
                        : point_scale_t<Fp2Ops>((Affine<Fp2Ops> *)pts, n, s, st);
}

}  // namespace

int point_fft(Context &c, int group, void *pts, uint32_t log_n, int mode, hipStream_t st) {
  return group == BH_G1 ? point_fft_t<FpOps>(c, pts, log_n, mode, st) : point_fft_t<Fp2Ops>(c, pts, log_n, mode, st);
}
// pts[i] *= g^i: the powers in a pool vector, then one scalar multiplication per point; waits for the stream
int point_distribute_powers(Context &c, int group, void *pts, u64 n, const fr_t &g, hipStream_t st) {
  fr_t *pw = (fr_t *)c.pool.acquire(n * sizeof(fr_t));
  if (!pw) return BH_ERR_HIP;
  int rc = launch_gen_powers(pw, n, g, fr_one_host(), 0, st);
  if (rc == BH_OK) rc = point_scale(group, pts, n, pf_vec(pw), st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  c.pool.release(pw);
  return rc;
}
int point_divide_by_z(int group, void *pts, uint32_t log_n, hipStream_t st) {
  return point_scale(group, pts, (u64)1 << log_n, pf_const(zinv_host(log_n)), st);
}
int point_mul_assign(int group, void *pts, const void *scalars_mont, u64 n, hipStream_t st) {
  return point_scale(group, pts, n, pf_vec((const fr_t *)scalars_mont), st);
}
int point_sub_assign(int group, void *a, const void *b, u64 n, hipStream_t st) {
  if (group == BH_G1)
    hipLaunchKernelGGL(pf_sub_kernel<FpOps>, dim3(pf_blocks(n)), dim3(PF_THREADS), 0, st, (Affine<FpOps> *)a,
                       (const Affine<FpOps> *)b, n);
  else
    hipLaunchKernelGGL(pf_sub_kernel<Fp2Ops>, dim3(pf_blocks(n)), dim3(PF_THREADS), 0, st, (Affine<Fp2Ops> *)a,
                       (const Affine<Fp2Ops> *)b, n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // namespace bh
