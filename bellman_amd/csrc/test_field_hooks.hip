// libbellman_hip_test.so: ONE field operation per element (or per lane group) on operands the caller chooses, raw results
// back (bh_test_field_ops_dev / _host of include/bellman_hip_test.h; tests/test_gpu_field_corners.py,
// tests/test_field_model_cpu.py).  Every operation goes through the function objects the kernels use (FpOps::mul is the
// out-of-line fp_mul_vec call, Fp2K3Ops::mul the leaf with its DPP exchange, ...); nothing is canonicalised on the way
// out.  The one-lane forms compile for the host too: the same `apply` runs in the kernel and in the host loop.
#include <string.h>

#include <utility>

#include "../../include/bellman_hip_test.h"
#include "final_exp.cuh"
#include "fp12.cuh"
#include "handles.hpp"
#include "msm_workers.cuh"
#include "point_read.cuh"

namespace bh {
namespace fieldops {

template <class T>
BH_HD T ld(const char *p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *(const T *)p;   // device buffers: 256-byte aligned allocations, strides that are multiples of 16
#else
  T v;
  memcpy(&v, p, sizeof v);
  return v;
#endif
}
template <class T>
BH_HD void st(char *p, const T &v) {
#ifdef __HIP_DEVICE_COMPILE__
  *(T *)p = v;
#else
  memcpy(p, &v, sizeof v);
#endif
}

// ---- forms 0 / 1: canonical Fe<P> ------------------------------------------------------------------------------------
template <class P>
struct CanonForm {
  typedef Fe<P> E;
  static constexpr int OPS = 10;
  static constexpr size_t RS = sizeof(E), AS = sizeof(E);
  static constexpr int arity(int op) { return (op == 0 || op == 1 || op == 4 || op == 5) ? 2 : 1; }
  static constexpr size_t r_bytes(int) { return RS; }
  template <int OP>
  BH_HD static void apply(char *r, u32 *flag, const char *a, const char *b, const char *, const char *) {
    const E x = ld<E>(a);
    E y, z;
    if (arity(OP) == 2) y = ld<E>(b); else fe_zero(y);
    switch (OP) {
      case 0: fe_add(z, x, y); break;
      case 1: fe_sub(z, x, y); break;
      case 2: fe_neg(z, x); break;
      case 3: fe_dbl(z, x); break;
      case 4: fe_mul(z, x, y); break;
      case 5: {   // the FFT's multiplier: second operand pre-sliced
        u32 B[Radix30<P>::L];
        fe_to_bform<P>(B, y);
        fe_mul_b<P>(z, x, B);
        break;
      }
      case 6: fe_sqr(z, x); break;
      case 7: fe_to_mont(z, x); break;
      case 8: fe_from_mont(z, x); break;
      default: fe_inv(z, x); break;
    }
    st(r, z);
    *flag = 0;
  }
};

// ---- forms 2 / 3: the lazily reduced function objects, one lane per element ------------------------------------------
template <class O>
struct LazyForm {
  typedef typename O::T E;
  static constexpr bool FP = O::WORDS == 12;
  static constexpr int OPS = FP ? 15 : 13;
  static constexpr size_t RS = sizeof(E), AS = sizeof(E);
  static constexpr int arity(int op) {
    return (op == 10 || op == 11 || op == 13 || op == 14) ? 4 : (op == 0 || op == 1 || op == 6 || op == 7 || op == 8) ? 2 : 1;
  }
  static constexpr size_t r_bytes(int op) { return op >= 13 ? 2 * RS : RS; }
  template <int OP>
  BH_HD static void apply(char *r, u32 *flag, const char *a, const char *b, const char *c, const char *d) {
    const E x = ld<E>(a);
    E y = x, v = x, w = x, z = x;
    if (arity(OP) >= 2) y = ld<E>(b);
    if (arity(OP) == 4) { v = ld<E>(c); w = ld<E>(d); }
    u32 f = 0;
    switch (OP) {
      case 0: O::add(z, x, y); break;
      case 1: O::sub(z, x, y); break;
      case 2: O::neg(z, x); break;
      case 3: O::dbl(z, x); break;
      case 4: O::canon(z); break;
      case 5: f = O::is_zero(x) ? 1u : 0u; break;
      case 6: f = O::eq(x, y) ? 1u : 0u; break;
      case 7: O::mul(z, x, y); break;
      case 8: O::mul_tail(z, x, y); break;
      case 9: O::sqr(z, x); break;
      case 10: O::mul2_sub(z, x, y, v, w); break;
      case 11: O::mul2_sub_tail(z, x, y, v, w); break;
      case 12: O::inv(z, x); break;
      default:
        if constexpr (FP) {   // two interleaved carry chains: (a, b) and (c, d)
          fp_t z1;
          if (OP == 13) fpl_add2(z, x, y, z1, v, w); else fpl_sub2(z, x, y, z1, v, w);
          st(r + RS, z1);
        }
        break;
    }
    st(r, z);
    *flag = f;
  }
};

// ---- form 6: the tower of fp12.cuh.  Every operand and every result sits in a 576-byte slot (an Fp12 value); an
// operation reads as much of a slot as its argument type needs ----------------------------------------------------
struct TowerForm {
  static constexpr int OPS = 22;
  static constexpr size_t RS = sizeof(fp12_t), AS = sizeof(fp12_t);
  static constexpr int arity(int op) { return op == 13 ? 4 : op == 7 ? 3 : (op == 1 || op == 6 || op == 8 || op == 11) ? 2 : 1; }
  static constexpr size_t r_bytes(int) { return RS; }
  template <int OP>
  BH_HD static void apply(char *r, u32 *flag, const char *a, const char *b, const char *c, const char *d) {
    u32 f = 0;
    if constexpr (OP <= 5) {
      const fp2_t x = ld<fp2_t>(a);
      fp2_t z;
      if (OP == 0) f2_mul_xi(z, x);
      else if (OP == 1) f2_mul_fp(z, x, ld<fp_t>(b));
      else if (OP == 2) f2_conj(z, x);
      else f2_mul_small(z, x, OP == 3 ? 3 : OP == 4 ? 4 : 12);
      st(r, z);
    } else if constexpr (OP <= 10) {
      const fp6_t x = ld<fp6_t>(a);
      fp6_t z;
      if (OP == 6) f6_mul(z, x, ld<fp6_t>(b));
      else if (OP == 7) f6_mul_01(z, x, ld<fp2_t>(b), ld<fp2_t>(c));
      else if (OP == 8) f6_mul_1(z, x, ld<fp2_t>(b));
      else if (OP == 9) f6_mul_v(z, x);
      else f6_inv(z, x);
      st(r, z);
    } else {
      const fp12_t x = ld<fp12_t>(a);
      fp12_t z = x;
      switch (OP) {
        case 11: f12_mul(z, x, ld<fp12_t>(b)); break;
        case 12: f12_sqr(z, x); break;
        case 13: f12_mul_line(z, ld<fp2_t>(b), ld<fp2_t>(c), ld<fp2_t>(d)); break;
        case 14: f12_inv(z, x); break;
        case 15: f12_conj(z, x); break;
        case 16: f12_frob1(z, x); break;
        case 17: f12_frob2(z, x); break;
        case 18: f12_cyc_sqr(z, x); break;
        case 20: f = f12_is_one(x) ? 1u : 0u; break;
#ifndef __HIP_DEVICE_COMPILE__   // on the device these two are the kernel chains of final_exp.cuh (tower_chain below)
        case 19: f12_cyc_exp_x(z, x); break;
        case 21: f12_final_exp(z, x); f12_canon(z); f = f12_is_one(z) ? 1u : 0u; break;
#endif
        default: break;
      }
      st(r, z);
    }
    *flag = f;
  }
};

// ---- form 7: the square roots and their helpers (point_read.cuh); 96-byte slots (an Fp2 value) -----------------------
struct SqrtForm {
  static constexpr int OPS = 5;
  static constexpr size_t RS = sizeof(fp2_t), AS = sizeof(fp2_t);
  static constexpr int arity(int) { return 1; }
  static constexpr size_t r_bytes(int) { return RS; }
  template <int OP>
  BH_HD static void apply(char *r, u32 *flag, const char *a, const char *, const char *, const char *) {
    fp2_t x = ld<fp2_t>(a), z = x;
    u32 f = 0;
    switch (OP) {
      case 0: f = fp_sqrt(z.c0, x.c0) ? 1u : 0u; break;
      case 1: f = fp2_sqrt(z, x) ? 1u : 0u; break;
      case 2: fpl_half(z.c0, x.c0); break;
      case 3: f = fp_lex_largest(x.c0) ? 1u : 0u; break;
      default: f = fp2_lex_largest(x) ? 1u : 0u; break;
    }
    st(r, z);
    *flag = f;
  }
};

template <class FORM, int OP>
__global__ __launch_bounds__(64) void field_op_kernel(char *r, u32 *flags, const char *a, const char *b, const char *c,
                                                      const char *d, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o = (size_t)i * FORM::AS;
  FORM::template apply<OP>(r + (size_t)i * FORM::r_bytes(OP), flags + i, a + o, b ? b + o : nullptr, c ? c + o : nullptr,
                           d ? d + o : nullptr);
}
template <class FORM, int OP>
static void field_op_host(char *r, u32 *flags, const char *a, const char *b, const char *c, const char *d, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const size_t o = i * FORM::AS;
    FORM::template apply<OP>(r + i * FORM::r_bytes(OP), flags + i, a + o, b ? b + o : nullptr, c ? c + o : nullptr,
                             d ? d + o : nullptr);
  }
}
typedef void (*dev_fn)(char *, u32 *, const char *, const char *, const char *, const char *, u32);
typedef void (*host_fn)(char *, u32 *, const char *, const char *, const char *, const char *, size_t);
template <class FORM, int... OP>
static dev_fn dev_entry(int op, std::integer_sequence<int, OP...>) {
  static const dev_fn t[] = {field_op_kernel<FORM, OP>...};
  return t[op];
}
template <class FORM, int... OP>
static host_fn host_entry(int op, std::integer_sequence<int, OP...>) {
  static const host_fn t[] = {field_op_host<FORM, OP>...};
  return t[op];
}
static bool have_operands(int arity, const void *a, const void *b, const void *c, const void *d) {
  return a && (arity < 2 || b) && (arity < 3 || c) && (arity < 4 || d);
}
template <class FORM>
static int run_dev(hipStream_t st, int op, void *r, u32 *flags, const void *a, const void *b, const void *c, const void *d, size_t n) {
  if (op < 0 || op >= FORM::OPS || !r || !flags || !have_operands(FORM::arity(op), a, b, c, d)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  const int ar = FORM::arity(op);
  hipLaunchKernelGGL(dev_entry<FORM>(op, std::make_integer_sequence<int, FORM::OPS>()), dim3((u32)((n + 63) / 64)), dim3(64), 0,
                     st, (char *)r, flags, (const char *)a, ar >= 2 ? (const char *)b : nullptr, ar >= 3 ? (const char *)c : nullptr,
                     ar >= 4 ? (const char *)d : nullptr, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
template <class FORM>
static int run_host(int op, void *r, u32 *flags, const void *a, const void *b, const void *c, const void *d, size_t n) {
  if (op < 0 || op >= FORM::OPS || !r || !flags || !have_operands(FORM::arity(op), a, b, c, d)) return BH_ERR_INVALID_ARG;
  const int ar = FORM::arity(op);
  host_entry<FORM>(op, std::make_integer_sequence<int, FORM::OPS>())((char *)r, flags, (const char *)a,
                                                                    ar >= 2 ? (const char *)b : nullptr,
                                                                    ar >= 3 ? (const char *)c : nullptr,
                                                                    ar >= 4 ? (const char *)d : nullptr, n);
  return BH_OK;
}

// f12_cyc_exp_x / f12_final_exp as the verifier runs them: the kernel chains of final_exp.cuh
__global__ __launch_bounds__(64) void flags_zero_kernel(u32 *flags, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = 0;
}
static int tower_chain(Context &c, int op, void *r, u32 *flags, const void *a, size_t n) {
  if (!r || !flags || !a) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  bool ok;
  if (op == 19) {
    hipLaunchKernelGGL(flags_zero_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, c.stream, flags, (u32)n);
    ok = exp_x_chain(c.stream, (const fp12_t *)a, (fp12_t *)r, (u32)n) && hipGetLastError() == hipSuccess;
  } else {
    fp12_t *ws = (fp12_t *)c.pool.acquire(4 * n * sizeof(fp12_t));
    if (!ws) return BH_ERR_HIP;
    ok = final_exp_chain(c.stream, (const fp12_t *)a, (fp12_t *)r, flags, ws, (u32)n);
    if (hipStreamSynchronize(c.stream) != hipSuccess) ok = false;
    c.pool.release(ws);
  }
  return ok ? BH_OK : BH_ERR_HIP;
}

// ---- forms 4 / 5: Fp2 on lane triples / lane pairs, with the kernels' own lane mapping (as lanes_group_law_kernel of
// test_hooks.hip).  raw[i * LANES + role] = what each lane of element i holds after the operation (the sum lane of a
// triple included), flags likewise (a predicate must come out the same in every lane of a group), stored[i] = what
// F::store writes.  Operation numbers as the one-lane forms; 13 = load / store round trip, 14 = one, 15 = curve_b ------
constexpr bool lanes_op_ok(int op) { return (op >= 0 && op <= 7) || op == 9 || (op >= 13 && op <= 15); }
constexpr int lanes_arity(int op) { return (op == 0 || op == 1 || op == 6 || op == 7) ? 2 : 1; }
template <class F, int OP>
__global__ __launch_bounds__(128) void lanes_field_op_kernel(fp_t *raw, fp2_t *stored, u32 *flags, const fp2_t *a, const fp2_t *b, u32 n) {
  u32 in_block, i;
  if (!worker_index<F>(default_per_wave<F>(), in_block, i) || i >= n) return;
  const u32 role = worker_role<F>();
  fp_t x, y, z;
  F::load(x, a + i);
  if (lanes_arity(OP) == 2) F::load(y, b + i); else y = x;
  z = x;
  u32 f = 0;
  switch (OP) {
    case 0: F::add(z, x, y); break;
    case 1: F::sub(z, x, y); break;
    case 2: F::neg(z, x); break;
    case 3: F::dbl(z, x); break;
    case 4: F::canon(z); break;
    case 5: f = F::is_zero(x) ? 1u : 0u; break;
    case 6: f = F::eq(x, y) ? 1u : 0u; break;
    case 7: F::mul(z, x, y); break;
    case 9: F::sqr(z, x); break;
    case 14: F::one(z); break;
    case 15: F::curve_b(z); break;
    default: break;   // 13: what was loaded is stored
  }
  raw[(size_t)i * F::LANES + role] = z;
  flags[(size_t)i * F::LANES + role] = f;
  F::store(&stored[i], z);
}
template <class F, int... OP>
static auto lanes_entry(int op, std::integer_sequence<int, OP...>) {
  typedef void (*fn)(fp_t *, fp2_t *, u32 *, const fp2_t *, const fp2_t *, u32);
  static const fn t[] = {lanes_field_op_kernel<F, OP>...};
  return t[op];
}
template <class F>
static int run_lanes(hipStream_t st, int op, void *r, u32 *flags, const void *a, const void *b, size_t n) {
  if (!lanes_op_ok(op) || !r || !flags || !a || (lanes_arity(op) == 2 && !b)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  const u32 wpb = workers_per_block<F>(128, default_per_wave<F>());
  fp_t *raw = (fp_t *)r;
  hipLaunchKernelGGL(lanes_entry<F>(op, std::make_integer_sequence<int, 16>()), dim3((u32)((n + wpb - 1) / wpb)), dim3(128), 0, st,
                     raw, (fp2_t *)(raw + n * F::LANES), flags, (const fp2_t *)a, (const fp2_t *)b, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

static int shape(int form, int op, size_t out[4]) {
  auto fill = [&](int ops, size_t r, size_t fl, size_t as, int ar) {
    if (op < 0 || op >= ops) return (int)BH_ERR_INVALID_ARG;
    out[0] = r; out[1] = fl; out[2] = as; out[3] = (size_t)ar;
    return (int)BH_OK;
  };
  switch (form) {
    case 0: return fill(CanonForm<FrParams>::OPS, 32, 1, 32, CanonForm<FrParams>::arity(op));
    case 1: return fill(CanonForm<FpParams>::OPS, 48, 1, 48, CanonForm<FpParams>::arity(op));
    case 2: return fill(LazyForm<FpOps>::OPS, LazyForm<FpOps>::r_bytes(op), 1, 48, LazyForm<FpOps>::arity(op));
    case 3: return fill(LazyForm<Fp2Ops>::OPS, 96, 1, 96, LazyForm<Fp2Ops>::arity(op));
    case 4: return lanes_op_ok(op) ? fill(16, 3 * 48 + 96, 3, 96, lanes_arity(op)) : (int)BH_ERR_INVALID_ARG;
    case 5: return lanes_op_ok(op) ? fill(16, 2 * 48 + 96, 2, 96, lanes_arity(op)) : (int)BH_ERR_INVALID_ARG;
    case 6: return fill(TowerForm::OPS, 576, 1, 576, TowerForm::arity(op));
    case 7: return fill(SqrtForm::OPS, 96, 1, 96, 1);
    default: return BH_ERR_INVALID_ARG;
  }
}
}  // namespace fieldops
}  // namespace bh

using namespace bh;
using namespace bh::fieldops;
extern "C" {
int bh_test_field_ops_shape(int form, int op, size_t out4[4]) { return out4 ? shape(form, op, out4) : BH_ERR_INVALID_ARG; }
int bh_test_field_ops_dev(bh_ctx *ctx, int form, int op, void *r_dev, uint32_t *flags_dev, const void *a_dev, const void *b_dev,
                          const void *c_dev, const void *d_dev, size_t n) {
  if (!ctx || n > (1u << 24)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = ctx->c.stream;
  int rc;
  switch (form) {
    case 0: rc = run_dev<CanonForm<FrParams>>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n); break;
    case 1: rc = run_dev<CanonForm<FpParams>>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n); break;
    case 2: rc = run_dev<LazyForm<FpOps>>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n); break;
    case 3: rc = run_dev<LazyForm<Fp2Ops>>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n); break;
    case 4: rc = run_lanes<Fp2K3Ops>(st, op, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 5: rc = run_lanes<Fp2PairOps>(st, op, r_dev, flags_dev, a_dev, b_dev, n); break;
    case 6:
      rc = (op == 19 || op == 21) ? tower_chain(ctx->c, op, r_dev, flags_dev, a_dev, n)
                                  : run_dev<TowerForm>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n);
      break;
    case 7: rc = run_dev<SqrtForm>(st, op, r_dev, flags_dev, a_dev, b_dev, c_dev, d_dev, n); break;
    default: return BH_ERR_INVALID_ARG;
  }
  if (rc == BH_OK) BH_HIP_CHECK(hipStreamSynchronize(st));
  return rc;
}
int bh_test_field_ops_host(int form, int op, void *r, uint32_t *flags, const void *a, const void *b, const void *c, const void *d,
                           size_t n) {
  switch (form) {
    case 0: return run_host<CanonForm<FrParams>>(op, r, flags, a, b, c, d, n);
    case 1: return run_host<CanonForm<FpParams>>(op, r, flags, a, b, c, d, n);
    case 2: return run_host<LazyForm<FpOps>>(op, r, flags, a, b, c, d, n);
    case 3: return run_host<LazyForm<Fp2Ops>>(op, r, flags, a, b, c, d, n);
    case 6: return run_host<TowerForm>(op, r, flags, a, b, c, d, n);
    case 7: return run_host<SqrtForm>(op, r, flags, a, b, c, d, n);
    default: return BH_ERR_INVALID_ARG;   // the lane forms exist on the device only
  }
}
}  // extern "C"
