// libbellman_hip_test.so: ONE group operation per worker on raw projective operands the caller chooses, raw results back
// (bh_test_group_ops_dev / _host of include/bellman_hip_test.h; tests/test_gpu_group_law.py, tests/test_group_model_cpu.py).
// Every operation goes through the functions the kernels call (xyzz_add / xyzz_madd / xyzz_dbl of ec.cuh, k2_add / k6_add,
// group_reduce_points / k2_group_reduce / k6_group_reduce and long_block_sum of msm_ec.cuh) with the kernels' own worker
// and lane mapping; nothing is canonicalised on the way out.  The one-lane forms compile for the host too: the same
// `apply` runs in the kernel and in the host loop, and the host trees add in the order of the shuffle trees.
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_ec.cuh"

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

template <class F, int OP>
__global__ __launch_bounds__(128) void group_op_kernel(XYZZ<typename F::Mem> *r, u32 *flags, const XYZZ<typename F::Mem> *a,
                                                       const void *b, u32 n) {
  typedef typename F::Mem M;
  u32 in_block, i;
  if (!worker_index<F>(default_per_wave<F>(), in_block, i) || i >= n) return;
  XYZZ<F> pa, pb, res;
  Affine<F> q;
  xyzz_set_identity(pa);
  xyzz_set_identity(pb);
  F::zero(q.x);
  F::zero(q.y);
  if (op_reads_a(OP)) load_xyzz<F>(pa, a + i);
  if (op_b_is_xyzz(OP)) load_xyzz<F>(pb, (const XYZZ<M> *)b + i);
  if (op_b_is_affine(OP)) load_affine<F>(q, (const Affine<M> *)b + i);
  const u32 f = apply<F, OP>(res, pa, pb, q, op_b_is_affine(OP) ? (const u32 *)((const Affine<M> *)b + i) : nullptr);
  store_xyzz<F>(r + i, res);
  flags[(size_t)i * F::LANES + worker_role<F>()] = f;
}
// groups of G consecutive workers of one wavefront, as msm_sum_kernel folds them: r[g] = sum of a[g G .. g G + G)
template <class F>
__global__ __launch_bounds__(64) void group_tree_kernel(XYZZ<typename F::Mem> *r, u32 *flags, const XYZZ<typename F::Mem> *a, u32 G,
                                                        u32 n_groups) {
  u32 t, gid;
  const bool live = worker_index<F>(tree_per_wave<F>(), t, gid);
  const u32 g = gid / G, sub = gid & (G - 1);
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  if (live && g < n_groups) load_xyzz<F>(acc, a + gid);
  group_reduce_points<F>(acc, G, sub);   // every lane of the wavefront takes part in the shuffles
  const bool id = xyzz_is_identity(acc);
  if (live && sub == 0 && g < n_groups) {
    store_xyzz<F>(r + g, acc);
    flags[(size_t)g * F::LANES + worker_role<F>()] = id ? 1u : 0u;
  }
}

// ---- form 1: G1 on lane pairs ----------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(128) void k2_op_kernel(XYZZ<FpOps> *r, u32 *flags, const XYZZ<FpOps> *a, const XYZZ<FpOps> *b, u32 n) {
  const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (i >= n) return;
  HalfPt ha, hb, hr;
  k2_load(ha, a + i);
  if (OP == OP_LOAD_STORE) {
    hr = ha;
  } else {
    k2_load(hb, b + i);
    if (OP == OP_ADD) {
      k2_add(hr, ha, hb);
    } else {
      hr = ha;
      k2_add(hr, hr, hb);
    }
  }
  const bool id = k2_is_identity(hr);
  k2_store(r + i, hr);
  flags[(size_t)i * 2 + k2_role()] = id ? 1u : 0u;
}
__global__ __launch_bounds__(64) void k2_tree_kernel(XYZZ<FpOps> *r, u32 *flags, const XYZZ<FpOps> *a, u32 G, u32 n_groups) {
  const u32 gid = blockIdx.x * 32 + (threadIdx.x >> 1);   // as msm_sum_k2_kernel
  const u32 g = gid / G, sub = gid & (G - 1);
  HalfPt acc;
  k2_set_identity(acc);
  if (g < n_groups) k2_load(acc, a + gid);
  k2_group_reduce(acc, G, sub);
  const bool id = k2_is_identity(acc);
  if (sub == 0 && g < n_groups) {
    k2_store(r + g, acc);
    flags[(size_t)g * 2 + k2_role()] = id ? 1u : 0u;
  }
}

// ---- form 5: G2 on lane sextets --------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(256) void k6_op_kernel(XYZZ<Fp2Ops> *r, u32 *flags, const XYZZ<Fp2Ops> *a, const XYZZ<Fp2Ops> *b, u32 n) {
  const u32 t_in_wave = (k3_lane() * 43u) >> 8, wave = threadIdx.x >> 6;   // as msm_sum_k6_kernel
  const u32 i = (blockIdx.x * (blockDim.x >> 6) + wave) * K6_PER_WAVE + t_in_wave;
  if (t_in_wave >= K6_PER_WAVE || i >= n) return;
  HalfPt ha, hb, hr;
  k6_load(ha, a + i);
  if (OP == OP_LOAD_STORE) {
    hr = ha;
  } else {
    k6_load(hb, b + i);
    if (OP == OP_ADD) {
      k6_add(hr, ha, hb);
    } else {
      hr = ha;
      k6_add(hr, hr, hb);
    }
  }
  const bool id = k6_is_identity(hr);
  k6_store(r + i, hr);
  flags[(size_t)i * 6 + k6_lane_in_worker()] = id ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k6_tree_kernel(XYZZ<Fp2Ops> *r, u32 *flags, const XYZZ<Fp2Ops> *a, u32 G, u32 n_groups) {
  const u32 t_in_wave = (k3_lane() * 43u) >> 8, wave = threadIdx.x >> 6;
  const bool live = t_in_wave < K6_PER_WAVE;
  const u32 gid = (blockIdx.x * (blockDim.x >> 6) + wave) * K6_PER_WAVE + t_in_wave;
  const u32 g = gid / G, sub = gid & (G - 1);
  HalfPt acc;
  fe_zero(acc.u);
  fe_zero(acc.v);
  if (live && g < n_groups) k6_load(acc, a + gid);
  k6_group_reduce(acc, G, sub);
  const bool id = k6_is_identity(acc);
  if (live && sub == 0 && g < n_groups) {
    k6_store(r + g, acc);
    flags[(size_t)g * 6 + k6_lane_in_worker()] = id ? 1u : 0u;
  }
}

// ---- long_block_sum: one workgroup of LONG_THREADS per case, long_workers<WK>() records each ---------------------------
template <class WK>
__device__ __forceinline__ bool wk_identity_flag(const typename WK::Pt &p) {
  if constexpr (WK::LANES == 6) return k6_is_identity(p);
  else if constexpr (std::is_same<typename WK::Pt, HalfPt>::value) return k2_is_identity(p);
  else return xyzz_is_identity(p);
}
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
    const bool id = wk_identity_flag<WK>(acc);
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
static bool form_info(int form, FormInfo &fi) {
  switch (form) {
    case 0: fi = {1, 1, tree_per_wave<FpOps>()}; return true;
    case 1: fi = {1, 2, K2Worker::PER_WAVE}; return true;
    case 2: fi = {2, 1, tree_per_wave<Fp2Ops>()}; return true;
    case 3: fi = {2, 3, tree_per_wave<Fp2K3Ops>()}; return true;
    case 4: fi = {2, 2, tree_per_wave<Fp2PairOps>()}; return true;
    case 5: fi = {2, 6, K6_PER_WAVE}; return true;
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

template <class F, int... OP>
static auto op_entry(int op, std::integer_sequence<int, OP...>) {
  typedef void (*fn)(XYZZ<typename F::Mem> *, u32 *, const XYZZ<typename F::Mem> *, const void *, u32);
  static const fn t[] = {group_op_kernel<F, OP>...};
  return t[op];
}
template <class F, class WK>
static int run_generic(hipStream_t st, int op, u32 G, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  typedef XYZZ<typename F::Mem> Rec;
  if (op == OP_TREE) {
    const u32 pw = tree_per_wave<F>();
    hipLaunchKernelGGL(group_tree_kernel<F>, dim3((u32)((n * G + pw - 1) / pw)), dim3(64), 0, st, (Rec *)r, flags, (const Rec *)a, G, (u32)n);
  } else if (op == OP_BLOCK_SUM) {
    hipLaunchKernelGGL(block_sum_kernel<WK>, dim3((u32)n), dim3(LONG_THREADS), 0, st, (Rec *)r, flags, (const Rec *)a);
  } else {
    const u32 wpb = workers_per_block<F>(128, default_per_wave<F>());
    hipLaunchKernelGGL(op_entry<F>(op, std::make_integer_sequence<int, OP_LOAD_STORE>()), dim3((u32)((n + wpb - 1) / wpb)), dim3(128), 0,
                       st, (Rec *)r, flags, (const Rec *)a, b, (u32)n);
  }
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
static int run_k2(hipStream_t st, int op, u32 G, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  typedef XYZZ<FpOps> Rec;
  const dim3 grid((u32)((2 * n + 127) / 128)), block(128);
  if (op == OP_TREE)
    hipLaunchKernelGGL(k2_tree_kernel, dim3((u32)((n * G + 31) / 32)), dim3(64), 0, st, (Rec *)r, flags, (const Rec *)a, G, (u32)n);
  else if (op == OP_BLOCK_SUM)
    hipLaunchKernelGGL(block_sum_kernel<K2Worker>, dim3((u32)n), dim3(LONG_THREADS), 0, st, (Rec *)r, flags, (const Rec *)a);
  else if (op == OP_ADD)
    hipLaunchKernelGGL(k2_op_kernel<OP_ADD>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  else if (op == OP_ADD_ALIAS)
    hipLaunchKernelGGL(k2_op_kernel<OP_ADD_ALIAS>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  else
    hipLaunchKernelGGL(k2_op_kernel<OP_LOAD_STORE>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
static int run_k6(hipStream_t st, int op, u32 G, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  typedef XYZZ<Fp2Ops> Rec;
  const u32 wpb = (256 / 64) * K6_PER_WAVE;
  const dim3 grid((u32)((n + wpb - 1) / wpb)), block(256);
  if (op == OP_TREE)
    hipLaunchKernelGGL(k6_tree_kernel, dim3((u32)((n * G + wpb - 1) / wpb)), block, 0, st, (Rec *)r, flags, (const Rec *)a, G, (u32)n);
  else if (op == OP_BLOCK_SUM)
    hipLaunchKernelGGL(block_sum_kernel<K6Worker>, dim3((u32)n), dim3(LONG_THREADS), 0, st, (Rec *)r, flags, (const Rec *)a);
  else if (op == OP_ADD)
    hipLaunchKernelGGL(k6_op_kernel<OP_ADD>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  else if (op == OP_ADD_ALIAS)
    hipLaunchKernelGGL(k6_op_kernel<OP_ADD_ALIAS>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  else
    hipLaunchKernelGGL(k6_op_kernel<OP_LOAD_STORE>, grid, block, 0, st, (Rec *)r, flags, (const Rec *)a, (const Rec *)b, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
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
    case 0: rc = run_generic<FpOps, XyzzWorker<FpOps>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 1: rc = run_k2(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 2: rc = run_generic<Fp2Ops, XyzzWorker<Fp2Ops>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 3: rc = run_generic<Fp2K3Ops, XyzzWorker<Fp2K3Ops>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 4: rc = run_generic<Fp2PairOps, XyzzWorker<Fp2PairOps>>(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
    default: rc = run_k6(st, op, G, r_dev, flags_dev, a_dev, b_dev, n); break;
  }
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(st));
  return rc;
}
int bh_test_group_ops_host(int form, int op, unsigned G, void *r, uint32_t *flags, const void *a, const void *b, size_t n) {
  if ((form != 0 && form != 2) || !args_ok(form, op, G, r, flags, a, b)) return BH_ERR_INVALID_ARG;   // the lane forms: device only
  return form == 0 ? run_host<FpOps>(op, G, r, flags, a, b, n) : run_host<Fp2Ops>(op, G, r, flags, a, b, n);
}
}  // extern "C"
