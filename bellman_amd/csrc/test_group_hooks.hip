// libbellman_hip_test.so: ONE group operation per worker on raw projective operands the caller chooses, raw results back
// (bh_test_group_ops_dev / _host of include/bellman_hip_test.h; tests/test_gpu_group_law.py, tests/test_group_model_cpu.py).
// Every operation goes through the functions the kernels call (xyzz_add / xyzz_madd / xyzz_dbl of ec.cuh, half_add,
// group_reduce_points / half_group_reduce and long_block_sum of msm_sums.cuh and msm_merge.cuh) through the kernels' own worker policies
// (XyzzWorker<F>, HalfWorker<P>); nothing is canonicalised on the way out.  The one-lane forms compile for the host too: the
// same `apply` runs in the kernel and in the host loop, and the host trees add in the order of the shuffle trees.
// bh_test_sum_jobs_dev runs msm_sum_kernel itself (tests/test_gpu_sum_jobs.py).
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_merge.cuh"

namespace bh {
namespace groupops {

enum {
  OP_ADD, OP_ADD_ALIAS, OP_MADD, OP_MADD_PREFETCH, OP_DBL, OP_DBL_AFFINE, OP_FROM_AFFINE, OP_TO_AFFINE, OP_IS_IDENTITY,
  OP_LOAD_STORE, OP_TREE, OP_BLOCK_SUM, N_OPS
};
constexpr bool op_reads_a(int op) { return op != OP_DBL_AFFINE && op != OP_FROM_AFFINE; }
constexpr bool op_b_is_xyzz(int op) { return op == OP_ADD || op == OP_ADD_ALIAS; }
constexpr bool op_b_is_affine(int op) { return op == OP_MADD || op == OP_MADD_PREFETCH || op == OP_DBL_AFFINE || op == OP_FROM_AFFINE; }
constexpr bool is_pow2(u32 g) { return g && !(g & (g - 1)); }

// flag word: bit 0 = the result is the identity as the code under test sees it, bit 1 = what xyzz_madd returned,
// bits 4-7 = how often the prefetch functor ran, bits 16-31 = the low half of the word it loaded
template <class F, int OP>
BH_HD u32 apply(XYZZ<F> &res, const XYZZ<F> &pa, const XYZZ<F> &pb, const Affine<F> &q, const u32 *touch) {
  u32 f = 0;
  if constexpr (OP == OP_ADD) {
    xyzz_add(res, pa, pb);
  } else if constexpr (OP == OP_ADD_ALIAS) {
    res = pa;
    xyzz_add(res, res, pb);
  } else if constexpr (OP == OP_MADD) {   // as the accumulation kernels: an identity base is skipped by the caller
    res = pa;
    if (!aff_is_identity(q)) f |= xyzz_madd(res, q) ? 2u : 0u;
  } else if constexpr (OP == OP_MADD_PREFETCH) {
    res = pa;
    u32 calls = 0, got = 0;
    auto prefetch = [&]() {
      got = *(const volatile u32 *)touch;
      calls++;
    };
    if (aff_is_identity(q)) prefetch(); else f |= xyzz_madd(res, q, prefetch) ? 2u : 0u;
    f |= (calls & 15u) << 4 | (got & 0xffffu) << 16;
  } else if constexpr (OP == OP_DBL) {
    xyzz_dbl(res, pa);
  } else if constexpr (OP == OP_DBL_AFFINE) {
    xyzz_dbl_affine(res, q);
  } else if constexpr (OP == OP_FROM_AFFINE) {
    xyzz_from_affine(res, q);
  } else if constexpr (OP == OP_TO_AFFINE) {
    if constexpr (F::LANES == 1) {   // (the lane bundles have no inversion: no kernel converts in those forms)
      Affine<F> t;
      xyzz_to_affine(t, pa);
      res.x = t.x;
      res.y = t.y;
      F::zero(res.zz);
      F::zero(res.zzz);
      return aff_is_identity(t) ? 1u : 0u;
    }
  } else {   // OP_IS_IDENTITY
    res = pa;
  }
  return f | (xyzz_is_identity(res) ? 1u : 0u);
}

// the same for a half-point worker (forms 1 and 5), which has the three operations its kernels use
template <class P, int OP>
__device__ __forceinline__ u32 apply_half(HalfPt &res, const HalfPt &pa, const HalfPt &pb) {
  res = pa;
  if constexpr (OP == OP_ADD) half_add<P>(res, pa, pb);
  else if constexpr (OP == OP_ADD_ALIAS) half_add<P>(res, res, pb);
  return half_is_identity<P>(res) ? 1u : 0u;
}

// false for lanes that carry no worker; `gid` = the worker's index over the whole launch
template <class WK>
__device__ __forceinline__ bool worker_global(u32 per_wave, u32 &gid) {
  u32 in_block;
  const bool live = WK::index(in_block, per_wave);
  gid = blockIdx.x * (blockDim.x >> 6) * per_wave + in_block;
  return live;
}
template <class WK, int OP>
__global__ __launch_bounds__(128) void group_op_kernel(XYZZ<typename WK::Mem> *r, u32 *flags, const XYZZ<typename WK::Mem> *a,
                                                       const void *b, u32 n) {
  typedef typename WK::Mem M;
  u32 i;
  if (!worker_global<WK>(WK::SOLO_PER_WAVE, i) || i >= n) return;
  typename WK::Pt pa, pb, res;
  WK::identity(pa);
  WK::identity(pb);
  if (op_reads_a(OP)) WK::load(pa, a + i);
  if (op_b_is_xyzz(OP)) WK::load(pb, (const XYZZ<M> *)b + i);
  u32 f;
  if constexpr (std::is_same<typename WK::Pt, HalfPt>::value) {
    f = apply_half<typename WK::Half, OP>(res, pa, pb);
  } else {
    typedef typename WK::Ops F;
    Affine<F> q;
    F::zero(q.x);
    F::zero(q.y);
    if (op_b_is_affine(OP)) load_affine<F>(q, (const Affine<M> *)b + i);
    f = apply<F, OP>(res, pa, pb, q, op_b_is_affine(OP) ? (const u32 *)((const Affine<M> *)b + i) : nullptr);
  }
  WK::store(r + i, res);
  flags[(size_t)i * WK::LANES + WK::role()] = f;
}
// groups of G consecutive workers of one wavefront, as msm_sum_kernel folds them: r[g] = sum of a[g G .. g G + G)
template <class WK>
__global__ __launch_bounds__(64) void group_tree_kernel(XYZZ<typename WK::Mem> *r, u32 *flags, const XYZZ<typename WK::Mem> *a, u32 G,
                                                        u32 n_groups) {
  u32 gid;
  const bool live = worker_global<WK>(WK::PER_WAVE, gid);
  const u32 g = gid / G, sub = gid & (G - 1);
  typename WK::Pt acc;
  WK::identity(acc);
  if (live && g < n_groups) WK::load(acc, a + gid);
  WK::tree(acc, G, sub);   // every lane of the wavefront takes part in the shuffles
  const bool id = WK::is_identity(acc);
  if (live && sub == 0 && g < n_groups) {
    WK::store(r + g, acc);
    flags[(size_t)g * WK::LANES + WK::role()] = id ? 1u : 0u;
  }
}

// ---- long_block_sum: one workgroup of LONG_THREADS per case, long_workers<WK>() records each ---------------------------
template <class WK>
__global__ __launch_bounds__(LONG_THREADS) void block_sum_kernel(XYZZ<typename WK::Mem> *r, u32 *flags, const XYZZ<typename WK::Mem> *a) {
  typedef typename WK::Pt Pt;
  __shared__ Pt wave_part[LONG_THREADS / 64][WK::LANES];
  u32 wid;
  const bool live = WK::index(wid);   // idle lanes stay for the barriers
  Pt acc;
  WK::identity(acc);
  if (live) WK::load(acc, a + (size_t)blockIdx.x * long_workers<WK>() + wid);
  long_block_sum<WK>(acc, live, wid, wave_part);
  if (live && wid == 0) {
    const bool id = WK::is_identity(acc);
    WK::store(r + blockIdx.x, acc);
    flags[(size_t)blockIdx.x * WK::LANES + WK::role()] = id ? 1u : 0u;
  }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------
struct FormInfo {
  int group;        // 1 or 2
  u32 lanes;        // flag words per worker
  u32 per_wave;     // workers of a wavefront in the trees
};
template <class WK>
static FormInfo info_of() { return {sizeof(XYZZ<typename WK::Mem>) == sizeof(XYZZ<FpOps>) ? 1 : 2, WK::LANES, WK::PER_WAVE}; }
static bool form_info(int form, FormInfo &fi) {
  switch (form) {
    case 0: fi = info_of<XyzzWorker<FpOps>>(); return true;
    case 1: fi = info_of<K2Worker>(); return true;
    case 2: fi = info_of<XyzzWorker<Fp2Ops>>(); return true;
    case 3: fi = info_of<XyzzWorker<Fp2K3Ops>>(); return true;
    case 4: fi = info_of<XyzzWorker<Fp2PairOps>>(); return true;
    case 5: fi = info_of<K6Worker>(); return true;
    default: return false;
  }
}
static bool op_ok(int form, int op) {
  if (op < 0 || op >= N_OPS) return false;
  if (op == OP_TREE || op == OP_BLOCK_SUM) return true;
  if (form == 1 || form == 5) return op == OP_ADD || op == OP_ADD_ALIAS || op == OP_LOAD_STORE;
  if (op == OP_LOAD_STORE) return false;
  return op != OP_TO_AFFINE || form == 0 || form == 2;
}
static bool args_ok(int form, int op, u32 G, const void *r, const void *flags, const void *a, const void *b) {
  FormInfo fi;
  if (!form_info(form, fi) || !op_ok(form, op) || !r || !flags) return false;
  if (op_reads_a(op) && !a) return false;
  if ((op_b_is_xyzz(op) || op_b_is_affine(op)) && !b) return false;
  if (op == OP_TREE && (!is_pow2(G) || G < 2 || G > fi.per_wave)) return false;
  return true;
}

template <class WK, int... OP>
static auto op_entry(int op, std::integer_sequence<int, OP...>) {
  typedef void (*fn)(XYZZ<typename WK::Mem> *, u32 *, const XYZZ<typename WK::Mem> *, const void *, u32);
  static const fn t[] = {group_op_kernel<WK, OP>...};
  return t[op];
}
template <class WK>
static int run_dev(hipStream_t st, int op, u32 G, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  typedef XYZZ<typename WK::Mem> Rec;
  if (op == OP_TREE) {
    const u32 pw = WK::PER_WAVE;
    hipLaunchKernelGGL(group_tree_kernel<WK>, dim3((u32)((n * G + pw - 1) / pw)), dim3(64), 0, st, (Rec *)r, flags, (const Rec *)a, G, (u32)n);
  } else if (op == OP_BLOCK_SUM) {
    hipLaunchKernelGGL(block_sum_kernel<WK>, dim3((u32)n), dim3(LONG_THREADS), 0, st, (Rec *)r, flags, (const Rec *)a);
  } else {
    const u32 wpb = (128 / 64) * WK::SOLO_PER_WAVE;
    hipLaunchKernelGGL(op_entry<WK>(op, std::make_integer_sequence<int, OP_TREE>()), dim3((u32)((n + wpb - 1) / wpb)), dim3(128), 0,
                       st, (Rec *)r, flags, (const Rec *)a, b, (u32)n);
  }
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// ---- msm_sum_kernel on its own: up to three jobs in one launch, counted and launched by sum_launch ------------------------
enum { SJ_MODE, SJ_GROUPS, SJ_COUNT, SJ_INNER, SJ_STRIDE, SJ_ISTRIDE, SJ_GROUP_SHIFT, SJ_SPLITS, SJ_LANES, SJ_IN_OFF, SJ_OUT_OFF, SJ_WORDS };
// every record a job reads lies inside [0, n_in), every output inside [0, n_out)
static bool sum_job_ok(const u32 *w, u32 max_lanes, size_t n_in, size_t n_out) {
  const u64 groups = w[SJ_GROUPS], count = w[SJ_COUNT], inner = w[SJ_INNER], splits = w[SJ_SPLITS], lanes = w[SJ_LANES];
  if (!groups || !count || !inner || !splits || count % splits || groups % splits || w[SJ_GROUP_SHIFT] > 24) return false;
  if (!is_pow2((u32)lanes) || lanes > max_lanes || w[SJ_OUT_OFF] + groups > n_out) return false;
  const u64 outer_max = (groups / splits - 1) / inner;
  u64 last;
  if (w[SJ_MODE] == SUM_STRIDED) last = (inner - 1) * w[SJ_ISTRIDE] + (count - 1) * w[SJ_STRIDE];
  else if (w[SJ_MODE] == SUM_BITS && is_pow2((u32)count) && splits == 1 && (1ull << inner) <= count) last = count - 1;
  else return false;
  return w[SJ_IN_OFF] + (outer_max << w[SJ_GROUP_SHIFT]) + last < n_in;
}
template <class WK, u32 NWAVES>
static int run_sum_jobs(hipStream_t st, const void *in, size_t n_in, void *out, size_t n_out, const u32 *words, size_t n_jobs) {
  typedef typename WK::Mem M;
  SumJobs<M> js{};
  for (size_t q = 0; q < 3; q++) {
    SumJob<M> &j = js.j[q];
    j.in = (const XYZZ<M> *)in;
    j.out = (XYZZ<M> *)out;
    j.d.groups = 0;
    j.d.lanes = 1;
    if (q >= n_jobs) continue;
    const u32 *w = words + q * SJ_WORDS;
    if (!sum_job_ok(w, NWAVES * WK::PER_WAVE, n_in, n_out)) return BH_ERR_INVALID_ARG;
    j.in += w[SJ_IN_OFF];
    j.out += w[SJ_OUT_OFF];
    j.d.mode = w[SJ_MODE]; j.d.groups = w[SJ_GROUPS]; j.d.count = w[SJ_COUNT]; j.d.inner = w[SJ_INNER];
    j.d.stride = w[SJ_STRIDE]; j.d.istride = w[SJ_ISTRIDE]; j.d.group_shift = w[SJ_GROUP_SHIFT];
    j.d.splits = w[SJ_SPLITS]; j.d.lanes = w[SJ_LANES];
  }
  return sum_launch<WK, NWAVES>(js, st) ? BH_OK : BH_ERR_HIP;
}

// ---- the host twins (forms 0 and 2) ------------------------------------------------------------------------------------
template <class T>
static T ld(const void *base, size_t i) {   // host buffers carry no alignment promise
  T v;
  memcpy(&v, (const char *)base + i * sizeof(T), sizeof v);
  return v;
}
template <class F, int OP>
static void host_op(char *r, u32 *flags, const char *a, const char *b, size_t n) {
  for (size_t i = 0; i < n; i++) {
    XYZZ<F> pa, pb, res;
    Affine<F> q;
    xyzz_set_identity(pa);
    xyzz_set_identity(pb);
    xyzz_set_identity(res);
    F::zero(q.x);
    F::zero(q.y);
    if (op_reads_a(OP)) pa = ld<XYZZ<F>>(a, i);
    if (op_b_is_xyzz(OP)) pb = ld<XYZZ<F>>(b, i);
    if (op_b_is_affine(OP)) q = ld<Affine<F>>(b, i);
    u32 word = 0;
    if (op_b_is_affine(OP)) memcpy(&word, b + i * sizeof(Affine<F>), 4);
    flags[i] = apply<F, OP>(res, pa, pb, q, &word);
    memcpy(r + i * sizeof res, &res, sizeof res);
  }
}
template <class F, int... OP>
static auto host_entry(int op, std::integer_sequence<int, OP...>) {
  typedef void (*fn)(char *, u32 *, const char *, const char *, size_t);
  static const fn t[] = {host_op<F, OP>...};
  return t[op];
}
// v[0] = v[0] + ... + v[G - 1] in the order of the shuffle trees: at distance off, worker sub < off adds worker sub + off
template <class F>
static void host_tree(XYZZ<F> *v, u32 G) {
  for (u32 off = G >> 1; off >= 1; off >>= 1)
    for (u32 sub = 0; sub < off; sub++) {
      XYZZ<F> t;
      xyzz_add(t, v[sub], v[sub + off]);
      v[sub] = t;
    }
}
template <class F>
static int run_host(int op, u32 G, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  typedef XYZZ<F> Rec;
  if (op == OP_TREE || op == OP_BLOCK_SUM) {
    // block_sum: G = workers per wavefront of the device form compared with (0: this form's own); LONG_THREADS / 64 wavefronts
    const u32 nw = LONG_THREADS / 64, pw = op == OP_TREE ? G : (G ? G : tree_per_wave<F>());
    if (op == OP_BLOCK_SUM && (!is_pow2(pw) || pw > 64)) return BH_ERR_INVALID_ARG;
    const size_t per = op == OP_TREE ? pw : (size_t)nw * pw;
    std::vector<Rec> v(per);
    for (size_t g = 0; g < n; g++) {
      memcpy(v.data(), (const char *)a + g * per * sizeof(Rec), per * sizeof(Rec));
      if (op == OP_TREE) {
        host_tree(v.data(), pw);
      } else {
        Rec part[nw];
        for (u32 w = 0; w < nw; w++) {
          host_tree(v.data() + (size_t)w * pw, pw);
          part[w] = v[(size_t)w * pw];
        }
        host_tree(part, nw);
        v[0] = part[0];
      }
      memcpy((char *)r + g * sizeof(Rec), &v[0], sizeof(Rec));
      flags[g] = xyzz_is_identity(v[0]) ? 1u : 0u;
    }
    return BH_OK;
  }
  host_entry<F>(op, std::make_integer_sequence<int, OP_LOAD_STORE>())((char *)r, flags, (const char *)a, (const char *)b, n);
  return BH_OK;
}
}  // namespace groupops
}  // namespace bh

using namespace bh;
using namespace bh::groupops;
extern "C" {
int bh_test_group_ops_shape(int form, int op, size_t out4[4]) {
  FormInfo fi;
  if (!out4 || !form_info(form, fi) || !op_ok(form, op)) return BH_ERR_INVALID_ARG;
  out4[0] = fi.group == 1 ? sizeof(XYZZ<FpOps>) : sizeof(XYZZ<Fp2Ops>);
  out4[1] = fi.lanes;
  out4[2] = fi.group == 1 ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  out4[3] = fi.per_wave;
  return BH_OK;
}
int bh_test_group_ops_dev(bh_ctx *ctx, int form, int op, unsigned G, void *r_dev, uint32_t *flags_dev, const void *a_dev,
                          const void *b_dev, size_t n) {
  if (!ctx || n > (1u << 22) || !args_ok(form, op, G, r_dev, flags_dev, a_dev, b_dev)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = ctx->c.stream;
  int rc;
  switch (form) {
    case 0: rc = run_dev<XyzzWorker<FpOps>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 1: rc = run_dev<K2Worker>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 2: rc = run_dev<XyzzWorker<Fp2Ops>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 3: rc = run_dev<XyzzWorker<Fp2K3Ops>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 4: rc = run_dev<XyzzWorker<Fp2PairOps>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    default: rc = run_dev<K6Worker>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
  }
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(st));
  return rc;
}
int bh_test_sum_jobs_dev(bh_ctx *ctx, int form, unsigned waves, const void *in_dev, size_t n_in, void *out_dev, size_t n_out,
                         const uint32_t *jobs, size_t n_jobs) {
  if (!ctx || !in_dev || !out_dev || !jobs || !n_jobs || n_jobs > 3 || n_in > (1u << 24) || n_out > (1u << 24)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = ctx->c.stream;
  int rc = BH_ERR_INVALID_ARG;
#define BH_SUM_FORM(FORM, WAVES, WK) \
  if (form == FORM && waves == WAVES) rc = run_sum_jobs<WK, WAVES>(st, in_dev, n_in, out_dev, n_out, jobs, n_jobs)
  BH_SUM_FORM(0, 1, XyzzWorker<FpOps>);
  BH_SUM_FORM(1, 1, K2Worker);
  BH_SUM_FORM(1, 2, K2Worker);
  BH_SUM_FORM(1, 4, K2Worker);
  BH_SUM_FORM(2, 1, XyzzWorker<Fp2Ops>);
  BH_SUM_FORM(3, 4, XyzzWorker<Fp2K3Ops>);
  BH_SUM_FORM(5, 4, K6Worker);
#undef BH_SUM_FORM
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(st));
  return rc;
}
int bh_test_group_ops_host(int form, int op, unsigned G, void *r, uint32_t *flags, const void *a, const void *b, size_t n) {
  if ((form != 0 && form != 2) || !args_ok(form, op, G, r, flags, a, b)) return BH_ERR_INVALID_ARG;   // the lane forms: device only
  return form == 0 ? run_host<FpOps>(op, G, r, flags, a, b, n) : run_host<Fp2Ops>(op, G, r, flags, a, b, n);
}
}  // extern "C"
