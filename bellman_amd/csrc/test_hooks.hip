// libbellman_hip_test.so: the test hooks of include/bellman_hip_test.h (field / group arithmetic on its own, the MSM
// sort stages, plan and shard-cut helpers) with the kernels only they use.  Links against libbellman_hip.so and is NOT
// part of the product: the shipped library exports exactly include/bellman_hip.h (tests/test_abi_cpu.py).
#include <string.h>

#include "../../include/bellman_hip_test.h"
#include "final_exp.cuh"
#include "fp12.cuh"
#include "msm_sums.cuh"
#include "pairing_launch.hpp"
#include "point_kernels.cuh"
#include "point_read.cuh"
#include "shard_cuts.hpp"
#include "fft_plan.hpp"
#include "fft_tables_plan.hpp"
#include "r1cs_dev.hpp"

namespace bh {
template <class P>
__global__ void fe_mul_kernel(Fe<P> *r, const Fe<P> *a, const Fe<P> *b, u64 n) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<P> x = a[i], y = b[i], z;
  fe_mul(z, x, y);
  r[i] = z;
}
template <class P>
static int test_fe_mul(void *r, const void *a, const void *b, u64 n, hipStream_t st) {
  if (!n) return BH_OK;
  hipLaunchKernelGGL(fe_mul_kernel<P>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (Fe<P> *)r, (const Fe<P> *)a,
                     (const Fe<P> *)b, n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
}  // namespace bh

// ---- test hook: the launch plan of a batched transform (host only; tests/test_fft_many_model_cpu.py) --------------------
int bh_test_fft_many_plan(uint32_t log_n, size_t k, size_t stride_elems, size_t scratch_vectors, int table_kind, uint64_t *out,
                          size_t cap) {
  if (log_n >= 32 || stride_elems < ((size_t)1 << log_n) || (log_n > 11 && !scratch_vectors) || (cap && !out)) return BH_ERR_INVALID_ARG;
  const bool one = table_kind == 1 && log_n >= 12 && log_n <= 24;
  const std::vector<bh::FftManyLaunch> plan = bh::fft_many_plan(log_n, k, stride_elems, scratch_vectors, one);
  for (size_t i = 0; i < plan.size() && i < cap; i++) {
    const bh::FftManyLaunch &l = plan[i];
    const uint64_t w[20] = {l.grid, l.threads, l.one_level, l.first_vec, l.n_vec, l.in_scratch, l.out_scratch, l.in_stride, l.out_stride,
                            l.geo.log_n, l.geo.s, l.geo.r, l.geo.log_c, l.geo.is_last, l.geo.r0, l.geo.L, l.geo.r1, l.geo.xcd_swizzle,
                            l.log_v, l.pass};
    memcpy(out + 20 * i, w, sizeof w);
  }
  return (int)plan.size();
}

// ---- test hook: the rules of the FFT table cache (host only; tests/test_fft_table_cache_cpu.py) ---------------------------
int bh_test_fft_table_policy(int rule, const uint64_t *in, size_t n_in, uint64_t *out) {
  if (!in || !out) return BH_ERR_INVALID_ARG;
  bh::FftHoldings h;
  if (rule == 0 || rule == 1) {
    if (n_in != (rule == 0 ? 11u : 4u)) return BH_ERR_INVALID_ARG;
    h.kind = (uint32_t)in[0]; h.roles = (uint32_t)in[1]; h.bytes = (size_t)in[2];
  }
  if (rule == 0) {
    if (in[3] >= 32) return BH_ERR_INVALID_ARG;
    uint32_t r[3] = {0, 0, 0}, L = 1;
    bh::plan_passes((uint32_t)in[3], r, &L);
    const bh::FftTableDecision d = bh::fft_tables_decide(h, (uint32_t)in[3], L, (int)in[4], in[5] != 0, in[6] != 0, in[7] != 0, (size_t)in[8],
                                                         (size_t)in[9], in[10] != 0);
    out[0] = d.evict_need; out[1] = d.kind; out[2] = d.roles; out[3] = d.bytes;
  } else if (rule == 1) {
    out[0] = bh::fft_tables_build_failed(h, (size_t)in[3]);
  } else if (rule == 2) {
    if (n_in < 4 || (n_in - 4) % 3) return BH_ERR_INVALID_ARG;
    std::vector<bh::FftCacheEntry> e;
    for (size_t i = 4; i < n_in; i += 3) e.push_back({(uint32_t)in[i], (size_t)in[i + 1], in[i + 2]});
    out[0] = (uint64_t)(int64_t)bh::fft_evict_victim(e.data(), e.size(), (uint32_t)in[0], (size_t)in[1], (size_t)in[2], (size_t)in[3]);
  } else {
    return BH_ERR_INVALID_ARG;
  }
  return BH_OK;
}

// ---- test hook: the group law in the multi-lane forms on its own (tests/test_gpu_parity.py::test_g2_k3_group_law,
// test_g2_lane_pair_group_law) --------------------------------------------------------------------------------
namespace bh {
template <class F>
__global__ __launch_bounds__(128) void lanes_group_law_kernel(XYZZ<Fp2Ops> *r_add, XYZZ<Fp2Ops> *r_madd, XYZZ<Fp2Ops> *r_dbl,
                                                              const Affine<Fp2Ops> *a, const Affine<Fp2Ops> *b, u32 n) {
  u32 in_block, i;
  if (!worker_index<F>(default_per_wave<F>(), in_block, i) || i >= n) return;
  Affine<F> pa, pb;
  load_affine<F>(pa, a + i);
  load_affine<F>(pb, b + i);
  XYZZ<F> x, y, z;
  xyzz_from_affine(x, pa);
  xyzz_from_affine(y, pb);
  xyzz_add(z, x, y);
  store_xyzz<F>(&r_add[i], z);
  z = x;
  if (!aff_is_identity(pb)) xyzz_madd(z, pb);
  store_xyzz<F>(&r_madd[i], z);
  xyzz_dbl(z, x);
  store_xyzz<F>(&r_dbl[i], z);
}
// out_*: n affine records each on the HOST (XYZZ results converted with the host arithmetic)
template <class F>
static int test_g2_lanes(Context &c, void *out_add, void *out_madd, void *out_dbl, const void *a_dev, const void *b_dev, u64 n) {
  typedef XYZZ<Fp2Ops> Pt;
  if (!n) return BH_OK;
  Pt *d = (Pt *)c.pool.acquire(3 * n * sizeof(Pt));
  if (!d) return BH_ERR_HIP;
  const u32 wpb = workers_per_block<F>(128, default_per_wave<F>());
  hipLaunchKernelGGL(lanes_group_law_kernel<F>, dim3((u32)((n + wpb - 1) / wpb)), dim3(128), 0, c.stream, d, d + n, d + 2 * n,
                     (const Affine<Fp2Ops> *)a_dev, (const Affine<Fp2Ops> *)b_dev, (u32)n);
  int rc = hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  std::vector<Pt> h(3 * n);
  if (rc == BH_OK && hipMemcpyAsync(h.data(), d, 3 * n * sizeof(Pt), hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  c.pool.release(d);
  if (rc != BH_OK) return rc;
  typedef HostFp2Ops H;
  void *outs[3] = {out_add, out_madd, out_dbl};
  for (int k = 0; k < 3; k++)
    for (u64 i = 0; i < n; i++) {
      Pt q = h[k * n + i];
      Fp2Ops::canon(q.x); Fp2Ops::canon(q.y); Fp2Ops::canon(q.zz); Fp2Ops::canon(q.zzz);   // lazily reduced on the device
      XYZZ<H> hq;
      memcpy(&hq, &q, sizeof hq);
      Affine<H> aff;
      xyzz_to_affine(aff, hq);
      memcpy((char *)outs[k] + i * sizeof aff, &aff, sizeof aff);
    }
  return BH_OK;
}
// the lane-sextet (K6) general addition of the merge kernels on its own: r[i] = a[i] + b[i], one sextet per pair of points
__global__ __launch_bounds__(64) void k6_add_kernel(XYZZ<Fp2Ops> *r, const Affine<Fp2Ops> *a, const Affine<Fp2Ops> *b, u32 n) {
  const u32 t = (k3_lane() * 43u) >> 8;
  const u32 i = blockIdx.x * K6_PER_WAVE + t;
  if (t >= K6_PER_WAVE || i >= n) return;
  const bool y = SextetHalf::side();
  auto from_affine = [&](HalfPt &h, const Affine<Fp2Ops> *p) {
    Fp2K3Ops::load(h.u, y ? &p->y : &p->x);
    fp_t ox, oy;
    Fp2K3Ops::load(ox, &p->x);
    Fp2K3Ops::load(oy, &p->y);
    if (Fp2K3Ops::is_zero_canonical(ox, oy)) { fe_zero(h.u); fe_zero(h.v); }   // the all-zero record is the identity
    else Fp2K3Ops::one(h.v);
  };
  HalfPt pa, pb;
  from_affine(pa, a + i);
  from_affine(pb, b + i);
  half_add<SextetHalf>(pa, pa, pb);
  SextetHalf::store(&r[i], pa);
}
static int test_g2_k6(Context &c, void *out_add, const void *a_dev, const void *b_dev, u64 n) {
  typedef XYZZ<Fp2Ops> Pt;
  if (!n) return BH_OK;
  Pt *d = (Pt *)c.pool.acquire(n * sizeof(Pt));
  if (!d) return BH_ERR_HIP;
  hipLaunchKernelGGL(k6_add_kernel, dim3((u32)((n + K6_PER_WAVE - 1) / K6_PER_WAVE)), dim3(64), 0, c.stream, d,
                     (const Affine<Fp2Ops> *)a_dev, (const Affine<Fp2Ops> *)b_dev, (u32)n);
  int rc = hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  std::vector<Pt> h(n);
  if (rc == BH_OK && hipMemcpyAsync(h.data(), d, n * sizeof(Pt), hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  c.pool.release(d);
  if (rc != BH_OK) return rc;
  typedef HostFp2Ops H;
  for (u64 i = 0; i < n; i++) {
    Pt q = h[i];
    Fp2Ops::canon(q.x); Fp2Ops::canon(q.y); Fp2Ops::canon(q.zz); Fp2Ops::canon(q.zzz);   // lazily reduced on the device
    XYZZ<H> hq;
    memcpy(&hq, &q, sizeof hq);
    Affine<H> aff;
    xyzz_to_affine(aff, hq);
    memcpy((char *)out_add + i * sizeof aff, &aff, sizeof aff);
  }
  return BH_OK;
}
static int test_g2_k3(Context &c, void *out_add, void *out_madd, void *out_dbl, const void *a_dev, const void *b_dev, u64 n) {
  return test_g2_lanes<Fp2K3Ops>(c, out_add, out_madd, out_dbl, a_dev, b_dev, n);
}
static int test_g2_pairs(Context &c, void *out_add, void *out_madd, void *out_dbl, const void *a_dev, const void *b_dev, u64 n) {
  return test_g2_lanes<Fp2PairOps>(c, out_add, out_madd, out_dbl, a_dev, b_dev, n);
}
}  // namespace bh

using namespace bh;
extern "C" {
int bh_test_shard_cuts(const size_t *lens, size_t n_shards, size_t skip, const uint64_t *density_words, size_t n_scalars,
                       size_t *cuts_out) {
  if (!lens || !n_shards || !cuts_out) return BH_ERR_INVALID_ARG;
  std::vector<size_t> cut, off;
  shard_cuts(lens, n_shards, skip, density_words, n_scalars, cut, off);
  memcpy(cuts_out, cut.data(), (n_shards + 1) * sizeof(size_t));
  return BH_OK;
}
size_t bh_test_pool_size_class(size_t bytes) { return DevicePool::size_class(bytes); }
int bh_test_fr_mul_dev(bh_ctx *ctx, void *r, const void *a, const void *b, size_t n) {
  int rc = test_fe_mul<FrParams>(r, a, b, n, ctx->c.stream);
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  return rc;
}
int bh_test_fp_mul_dev(bh_ctx *ctx, void *r, const void *a, const void *b, size_t n) {
  int rc = test_fe_mul<FpParams>(r, a, b, n, ctx->c.stream);
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  return rc;
}
int bh_test_point_add_dev(bh_ctx *ctx, int group, void *r, const void *a, const void *b, size_t n) {
  int rc = group == BH_G1 ? test_point_add_t<FpOps>(r, a, b, n, ctx->c.stream) : test_point_add_t<Fp2Ops>(r, a, b, n, ctx->c.stream);
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  return rc;
}
int bh_test_g2_k3_dev(bh_ctx *ctx, void *out_add_host, void *out_madd_host, void *out_dbl_host, const void *a_dev,
                      const void *b_dev, size_t n) {
  if (!ctx) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return test_g2_k3(ctx->c, out_add_host, out_madd_host, out_dbl_host, a_dev, b_dev, n);
}
int bh_test_g2_k6_dev(bh_ctx *ctx, void *out_add_host, const void *a_dev, const void *b_dev, size_t n) {
  if (!ctx) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return test_g2_k6(ctx->c, out_add_host, a_dev, b_dev, n);
}
int bh_test_g2_pairs_dev(bh_ctx *ctx, void *out_add_host, void *out_madd_host, void *out_dbl_host, const void *a_dev,
                         const void *b_dev, size_t n) {
  if (!ctx) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return test_g2_pairs(ctx->c, out_add_host, out_madd_host, out_dbl_host, a_dev, b_dev, n);
}
void bh_test_fr_mul_host(void *r, const void *a, const void *b, size_t n) {
  for (size_t i = 0; i < n; i++) fe_mul(((fr_t *)r)[i], ((const fr_t *)a)[i], ((const fr_t *)b)[i]);
}
void bh_test_fr_mul_bform_host(void *r, const void *a, const void *b, size_t n) {
  // the FFT's multiplier: second operand pre-sliced into 30-bit limbs (ff.cuh fe_to_bform / fe_mul_b)
  for (size_t i = 0; i < n; i++) {
    u32 B[9];
    fe_to_bform<FrParams>(B, ((const fr_t *)b)[i]);
    fe_mul_b<FrParams>(((fr_t *)r)[i], ((const fr_t *)a)[i], B);
  }
}
void bh_test_fp_mul_host(void *r, const void *a, const void *b, size_t n) {
  for (size_t i = 0; i < n; i++) fe_mul(((fp_t *)r)[i], ((const fp_t *)a)[i], ((const fp_t *)b)[i]);
}
void bh_test_fp_sqrt_host(void *r, unsigned char *ok, const void *a, size_t n) {
  for (size_t i = 0; i < n; i++) {
    fp_t x, y;
    memcpy(&x, (const char *)a + 48 * i, 48);
    ok[i] = fp_sqrt(y, x) ? 1 : 0;
    fpl_canon(y, y);
    memcpy((char *)r + 48 * i, &y, 48);
  }
}
void bh_test_fp2_sqrt_host(void *r, unsigned char *ok, const void *a, size_t n) {
  for (size_t i = 0; i < n; i++) {
    fp2_t x, y;
    memcpy(&x, (const char *)a + 96 * i, 96);
    ok[i] = fp2_sqrt(y, x) ? 1 : 0;
    Fp2Ops::canon(y);
    memcpy((char *)r + 96 * i, &y, 96);
  }
}
int bh_test_fp_lazy_host(int op, void *r, const void *a, const void *b) {
  // the lazily reduced Fp helpers of the curve code (ff.cuh), compiled for the host; operands in [0, 2p)
  fp_t x, y, z;
  memcpy(&x, a, sizeof x);
  if (b) memcpy(&y, b, sizeof y); else fe_zero(y);
  int flag = 0;
  switch (op) {
    case 0: fpl_add(z, x, y); break;
    case 1: fpl_sub(z, x, y); break;
    case 2: fpl_neg(z, x); break;
    case 3: fpl_canon(z, x); break;
    case 4: z = x; flag = fpl_is_zero(x) ? 1 : 0; break;
    case 5: z = fp_mul_call(x, y); break;   // lazily reduced Montgomery product
    case 6: z = fp_sqr_call(x); break;
    case 7: z = x; flag = fpl_eq(x, y) ? 1 : 0; break;
    default: return BH_ERR_INVALID_ARG;
  }
  memcpy(r, &z, sizeof z);
  return flag;
}
void bh_test_fr_inv_host(void *r, const void *a, size_t n) {
  for (size_t i = 0; i < n; i++) fe_inv(((fr_t *)r)[i], ((const fr_t *)a)[i]);
}
void bh_test_point_add_host(int group, void *r, const void *a, const void *b, size_t n) {
  if (group == BH_G1) devhdr_point_add_t<FpOps>(r, a, b, n); else devhdr_point_add_t<Fp2Ops>(r, a, b, n);
}
void bh_test_point_mul_host(int group, void *r, const void *a, const void *k) {
  if (group == BH_G1) devhdr_point_mul_t<FpOps>(r, a, (const u32 *)k); else devhdr_point_mul_t<Fp2Ops>(r, a, (const u32 *)k);
}
}  // extern "C"

// ---- test hook: full pairings (tests/test_gpu_verifier.py, tests/test_verifier_cpu.py) ------------------------------
namespace bh {
// (pairing_launch.hpp: the shipped launch functions of csrc/pairing_kernels.cuh, which test_pairing_hooks.hip compiles into
// this library)
// one pairing per lane; out = 12 canonical Fp (not Montgomery) in w-basis order w^0, w^1 (each c0 then c1 of Fp2), ...
BH_HD void pairing_one(fp12_t &r, const Affine<FpOps> &p, const Affine<Fp2Ops> &q, const line_t *lines) {
  fp12_t f;
  if (aff_is_identity(p) || aff_is_identity(q)) f12_one(f);
  else miller_loop_lines(f, p.x, p.y, [&](int k) { return lines[k]; });
  f12_final_exp(r, f);
  f12_canon(r);
}
BH_HD void gt_store_canonical(fp_t *out, const fp12_t &r) {
  for (int k = 0; k < 6; k++) {
    fe_from_mont(out[2 * k], f12_w(r, k).c0);
    fe_from_mont(out[2 * k + 1], f12_w(r, k).c1);
  }
}
__global__ __launch_bounds__(64) void test_gt_store_kernel(const fp12_t *r, fp_t *out, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  gt_store_canonical(out + 12 * (size_t)i, r[i]);
}
}  // namespace bh

extern "C" {
int bh_test_pairing(bh_ctx *ctx, size_t n, const void *g1_affine, const void *g2_affine, void *gt_out) {
  if (!ctx || (n && (!g1_affine || !g2_affine || !gt_out))) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  const size_t bl = n * MILLER_LINES * sizeof(line_t);
  char *d = (char *)c.pool.acquire(n * 96 + n * 192 + n * 576 + bl + 5 * n * sizeof(fp12_t) + n * sizeof(u32));
  if (!d) return BH_ERR_HIP;
  Affine<FpOps> *p = (Affine<FpOps> *)d;
  Affine<Fp2Ops> *q = (Affine<Fp2Ops> *)(d + n * 96);
  fp_t *out = (fp_t *)(d + n * 288);
  line_t *lines = (line_t *)(d + n * 864);
  int rc = BH_OK;
  if (hipMemcpyAsync(p, g1_affine, n * 96, hipMemcpyHostToDevice, c.stream) != hipSuccess ||
      hipMemcpyAsync(q, g2_affine, n * 192, hipMemcpyHostToDevice, c.stream) != hipSuccess)
    rc = BH_ERR_HIP;
  if (!rc) {
    const u32 nb = (u32)((n + 63) / 64);
    (void)hipGetLastError();
    fp12_t *f = (fp12_t *)(d + n * 864 + bl);
    u32 *qflags = (u32 *)(f + 5 * n);
    if (launch_g2_lines(c.stream, q, sizeof(Affine<Fp2Ops>), 0, lines, qflags, n) != BH_OK ||
        launch_miller(c.stream, p, lines, qflags, f, n, nullptr, nullptr, 0) != BH_OK ||
        !final_exp_chain(c.stream, f, f, nullptr, f + n, (u32)n))
      rc = BH_ERR_HIP;
    (void)hipGetLastError();
    hipLaunchKernelGGL(test_gt_store_kernel, dim3(nb), dim3(64), 0, c.stream, f, out, (u32)n);
    if (hipGetLastError() != hipSuccess) rc = BH_ERR_HIP;
  }
  if (!rc && hipMemcpyAsync(gt_out, out, n * 576, hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess && !rc) rc = BH_ERR_HIP;
  c.pool.release(d);
  return rc;
}
// the same arithmetic compiled for the host (toolchain-only tests of fp12.cuh)
void bh_test_pairing_host(size_t n, const void *g1_affine, const void *g2_affine, void *gt_out) {
  std::vector<line_t> lines(MILLER_LINES);
  for (size_t i = 0; i < n; i++) {
    Affine<FpOps> p;
    Affine<Fp2Ops> q;
    memcpy(&p, (const char *)g1_affine + 96 * i, 96);
    memcpy(&q, (const char *)g2_affine + 192 * i, 192);
    if (!aff_is_identity(q)) g2_lines(q.x, q.y, [&](int k, const line_t &l) { lines[k] = l; });
    fp12_t r;
    pairing_one(r, p, q, lines.data());
    gt_store_canonical((fp_t *)gt_out + 12 * i, r);
  }
}
}  // extern "C"

// the witness tile of the k-witness constraint kernels (r1cs.hip)
extern "C" uint32_t bh_test_r1cs_many_tile(void) { return bh::R1CS_MANY_TILE; }

// ---- test hooks of the witness solver: the planner on its own (host only; tests/test_r1cs_solve_model_cpu.py) and the
// launch forms of a solver (tests/test_gpu_r1cs_solve.py, tools/bench_r1cs_solve.py) ------------------------------------
extern "C" int bh_test_r1cs_solve_plan(size_t n_inputs, size_t n_aux, size_t n_constraints, const bh_csr abc[3], const void *coeffs,
                                       size_t n_coeffs, const bh_solver_desc *desc, uint32_t *first_unsolved, int64_t *definer,
                                       uint32_t *level, size_t counts5[5]) {
  using namespace bh;
  if (first_unsolved) *first_unsolved = SOLVE_NO_VAR;
  if (!abc || !coeffs || !n_coeffs || !desc) return BH_ERR_INVALID_ARG;
  SolveCsr m[3];
  for (int i = 0; i < 3; i++) m[i] = SolveCsr{abc[i].row_ptr, abc[i].var, abc[i].coeff};
  SolveDesc d;
  d.supplied = desc->supplied; d.n_supplied = desc->n_supplied;
  d.hints = reinterpret_cast<const SolveHint *>(desc->hints); d.n_hints = desc->n_hints;
  d.lc_var = desc->lc_var; d.lc_coeff = desc->lc_coeff; d.out_var = desc->out_var;
  d.n_lc = d.n_out = 0;
  for (size_t h = 0; h < desc->n_hints; h++) {
    if (desc->hints[h].lc_end > d.n_lc) d.n_lc = desc->hints[h].lc_end;
    if (desc->hints[h].out_end > d.n_out) d.n_out = desc->hints[h].out_end;
  }
  const SolvePlan<fr_t> p = solve_plan(SolveFr(), n_inputs + n_aux, n_constraints, m, (const fr_t *)coeffs, n_coeffs, d,
                                       (const fr_t *)desc->hint_coeffs, desc->n_hints ? desc->n_hint_coeffs : 0);
  if (first_unsolved) *first_unsolved = p.first_unsolved;
  if (p.status != SOLVE_OK) return p.status;
  for (size_t v = 0; v < n_inputs + n_aux; v++) {
    if (definer) definer[v] = p.by[v] == SOLVE_BY_NONE ? -1 : p.by[v] == SOLVE_BY_CONSTRAINT ? (int64_t)p.by_index[v] : -2 - (int64_t)p.by_index[v];
    if (level) level[v] = p.level[v];
  }
  if (counts5) {
    counts5[0] = p.n_supplied; counts5[1] = p.n_defined; counts5[2] = p.n_hinted;
    counts5[3] = p.level_ptr.size() - 1; counts5[4] = p.widest;
  }
  return BH_OK;
}
extern "C" int bh_test_r1cs_solver_tune(bh_r1cs_solver *s, uint32_t form, uint32_t witnesses_per_group, uint64_t level_min_items) {
  if (!s || form > bh::SOLVE_FORM_LEVEL) return BH_ERR_INVALID_ARG;
  s->force_form = form;
  s->force_w = witnesses_per_group;
  s->level_min_items = level_min_items ? level_min_items : bh::SOLVE_LEVEL_MIN_ITEMS;
  return BH_OK;
}

// ---- test hooks of the word-program witness generator: validator and host interpreter on their own (host only;
// tests/test_word_program_cpu.py) and the scratch chunk of a handle (tests/test_gpu_word_witness.py) --------------------------
extern "C" int bh_test_word_program(const bh_word_witness_desc *desc, uint32_t bad_index[2], const uint32_t *ext, void *inputs_out,
                                    void *aux_out, uint64_t *words_out) {
  using namespace bh;
  if (bad_index) { bad_index[0] = 0; bad_index[1] = WORD_NO_INDEX; }
  if (!desc) return BH_ERR_INVALID_ARG;
  const WordDesc &d = *reinterpret_cast<const WordDesc *>(desc);
  const WordProgram p = word_program_validate(d);
  if (p.status != WORD_OK) {
    if (bad_index) { bad_index[0] = p.bad_code; bad_index[1] = p.bad_index; }
    return p.status;
  }
  if (!ext && d.n_ext) return BH_OK;
  if (!inputs_out && !aux_out) return BH_OK;
  if (!inputs_out || (d.n_aux && !aux_out)) return BH_ERR_INVALID_ARG;
  word_program_interpret(WordFr(), d, p, ext, (fr_t *)inputs_out, (fr_t *)aux_out, words_out);
  return BH_OK;
}
extern "C" int bh_test_word_witness_chunk(bh_word_witness *w, size_t witnesses_per_chunk) {
  if (!w) return BH_ERR_INVALID_ARG;
  w->force_chunk = witnesses_per_chunk;
  return BH_OK;
}
