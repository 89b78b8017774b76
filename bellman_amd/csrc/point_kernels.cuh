// Point kernels outside the MSM pipeline - fixed-base multiplication, point addition, the group-membership check, the
// window table of a base vector - with their launch wrappers, and the host-side group helpers (instantiated per group by
// BH_INSTANTIATE_MSM_SUPPORT of msm_ec.cuh).
#pragma once
#include <string.h>

#include <vector>

#include "ec.cuh"
#include "host_fp.hpp"
#include "msm_scalar.cuh"
#include "msm_types.hpp"
#include "points.hpp"

namespace bh {

// ============================================================================================
// fixed-base scalar multiplication (fixture generation) and test hooks
// ============================================================================================
// out[i] = [s_i] base (generator.rs:271-296,398-421 use a windowed fixed-base table on the CPU; so does this).
// [r4] Table T[j][d - 1] = d * 2^(8j) * base, j < 32, d = 1 .. 255 (affine; 0.8 MB for G1, 1.6 MB for G2, L2 resident): a
// scalar is its 32 bytes, a multiplication is at most 32 mixed additions and no doubling at all - 320 field products
// and one inversion instead of the 255 doublings + ~127 additions (3 600 products) of the double-and-add ladder this
// replaces.  generate_parameters for a 2^20-constraint circuit is 4 x 2^20 G1 + 2^20 G2 such multiplications.
constexpr u32 FB_ROWS = 32, FB_COLS = 255;
// step 1: the row bases 2^(8j) * base (one lane per row: 8j doublings, one inversion)
template <class F>
__global__ void __launch_bounds__(64) fixed_base_rows_kernel(Affine<F> base, Affine<F> *table) {
  const u32 j = threadIdx.x;
  if (j >= FB_ROWS) return;
  Affine<F> p = base;
  if (j && !aff_is_identity(base)) {
    XYZZ<F> acc, t;
    xyzz_dbl_affine(acc, base);
    for (u32 k = 1; k < 8 * j; k++) { xyzz_dbl(t, acc); acc = t; }
    xyzz_to_affine(p, acc);
  }
  table[(size_t)j * FB_COLS] = p;
}
// step 2: d * (row base) for d = 2 .. 255 by double-and-add over the 8 bits of d (one lane per entry)
template <class F>
__global__ void __launch_bounds__(128) fixed_base_table_kernel(Affine<F> *table) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= FB_ROWS * FB_COLS) return;
  const u32 j = e / FB_COLS, d = e % FB_COLS + 1;
  if (d == 1) return;
  const Affine<F> p = table[(size_t)j * FB_COLS];
  Affine<F> r = p;
  if (!aff_is_identity(p)) {
    XYZZ<F> acc, t;
    xyzz_set_identity(acc);
    for (int b = 7; b >= 0; b--) {
      xyzz_dbl(t, acc);
      acc = t;
      if ((d >> b) & 1) xyzz_madd(acc, p);
    }
    xyzz_to_affine(r, acc);
  }
  table[e] = r;
}
template <class F>
__global__ void __launch_bounds__(128) fixed_base_mul_kernel(const Affine<F> *table, const void *scalars, int fmt, u64 n, Affine<F> *out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_t s;
  load_scalar(scalars, i, fmt, s);
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  for (u32 j = 0; j < FB_ROWS; j++) {
    const u32 d = (s.l[j >> 2] >> ((j & 3) * 8)) & 255u;
    if (!d) continue;
    const Affine<F> q = table[(size_t)j * FB_COLS + d - 1];
    if (!aff_is_identity(q)) xyzz_madd(acc, q);   // (an identity base gives an all-identity table)
  }
  Affine<F> r;
  xyzz_to_affine(r, acc);
  out[i] = r;
}
template <class F>
__global__ void __launch_bounds__(128) point_add_kernel(Affine<F> *r, const Affine<F> *a, const Affine<F> *b, u64 n) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  XYZZ<F> x, y, z;
  xyzz_from_affine(x, a[i]);
  xyzz_from_affine(y, b[i]);
  xyzz_add(z, x, y);
  Affine<F> o;
  xyzz_to_affine(o, z);
  r[i] = o;
}
// from_uncompressed's two group-membership tests (bls12_381: is_on_curve & is_torsion_free) for
// points the decode kernel already accepted: y^2 = x^3 + b, then [q]P = O by plain double-and-add
// (q is the same for every lane, so the loop does not diverge).  One-time CRS loading work.
template <class F>
__global__ void __launch_bounds__(64) point_check_kernel(const Affine<F> *pts, u64 n, u32 *status) {
  typedef typename F::T T;
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 st = status[i];
  if (st & (PT_INVALID_MASK | PT_IS_INF)) return;
  const Affine<F> p = pts[i];
  T lhs, rhs, b;
  F::sqr(lhs, p.y);
  F::sqr(rhs, p.x);
  F::mul(rhs, rhs, p.x);
  F::curve_b(b);
  F::add(rhs, rhs, b);
  if (!F::eq(lhs, rhs)) { status[i] = st | PT_OFF_CURVE; return; }
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  for (int bit = 254; bit >= 0; bit--) {
    XYZZ<F> t;
    xyzz_dbl(t, acc);
    acc = t;
    if ((FrParams::mod(bit >> 5) >> (bit & 31)) & 1) xyzz_madd(acc, p);
  }
  if (!xyzz_is_identity(acc)) status[i] = st | PT_NOT_IN_SUBGROUP;
}
// Window table of a registered base vector: row j holds 2^(c*j) P_i in affine form, so that digit j of
// a scalar can go to the same bucket set as digit 0 (one bucket reduction instead of W, no Horner
// over windows).  One lane per base walks the rows: c doublings and one inversion per row.  Lane i reads record i of `src`
// (src_stride bytes apart) and writes row j at dst + (j n + i) dst_stride: the table is built where and as it stays - at a
// 128-byte stride for the big G1 tables (api_bases.hip table_will_pad) - and the bytes between two records are never written.
template <class F>
__global__ void __launch_bounds__(128) window_table_kernel(const char *src, u32 src_stride, char *dst, u32 dst_stride, u64 n,
                                                           u32 c, u32 W) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> p = *reinterpret_cast<const Affine<F> *>(src + i * src_stride);
  for (u32 j = 0; j < W; j++) {
    if (j && !aff_is_identity(p)) {
      XYZZ<F> acc, t;
      xyzz_dbl_affine(acc, p);
      for (u32 k = 1; k < c; k++) { xyzz_dbl(t, acc); acc = t; }
      xyzz_to_affine(p, acc);
    }
    *reinterpret_cast<Affine<F> *>(dst + ((u64)j * n + i) * dst_stride) = p;
  }
}
template <class F>
static int window_table_t(BaseView src, void *dst, u32 dst_stride, u64 n, u32 c, u32 W, hipStream_t st) {
  const u32 blocks = (u32)((n + 127) / 128);
  if (!blocks) return BH_OK;
  if (src.stride < sizeof(Affine<F>) || dst_stride < sizeof(Affine<F>) || src.stride % 16 || dst_stride % 16) return BH_ERR_INVALID_ARG;
  hipLaunchKernelGGL(window_table_kernel<F>, dim3(blocks), dim3(128), 0, st, (const char *)src.ptr, src.stride, (char *)dst,
                     dst_stride, n, c, W);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
template <class F>
static int points_check_t(const void *pts_dev, u64 n, u32 *status_dev, hipStream_t st) {
  const u32 blocks = (u32)((n + 63) / 64);
  if (!blocks) return BH_OK;
  hipLaunchKernelGGL(point_check_kernel<F>, dim3(blocks), dim3(64), 0, st, (const Affine<F> *)pts_dev, n, status_dev);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// the 64-bit-limb host arithmetic over the same records (host_fp.hpp)
template <> struct HostOf<FpOps> { typedef HostFpOps type; };
template <> struct HostOf<Fp2Ops> { typedef HostFp2Ops type; };

template <class F>
static int fixed_base_mul_t(const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev,
                            hipStream_t st, void *table_dev) {
  const u32 blocks = (u32)((n + 127) / 128);
  if (!blocks) return BH_OK;
  Affine<F> b;
  memcpy(&b, base_host, sizeof b);
  Affine<F> *table = (Affine<F> *)table_dev;   // FB_ROWS * FB_COLS records, owned by the caller until `st` has drained
  hipLaunchKernelGGL(fixed_base_rows_kernel<F>, dim3(1), dim3(64), 0, st, b, table);
  BH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fixed_base_table_kernel<F>, dim3((FB_ROWS * FB_COLS + 127) / 128), dim3(128), 0, st, table);
  BH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fixed_base_mul_kernel<F>, dim3(blocks), dim3(128), 0, st, (const Affine<F> *)table, scalars_dev, fmt, n,
                     (Affine<F> *)out_dev);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
template <class F>
static int test_point_add_t(void *r, const void *a, const void *b, u64 n, hipStream_t st) {
  const u32 blocks = (u32)((n + 127) / 128);
  if (!blocks) return BH_OK;
  hipLaunchKernelGGL(point_add_kernel<F>, dim3(blocks), dim3(128), 0, st, (Affine<F> *)r, (const Affine<F> *)a,
                     (const Affine<F> *)b, n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// Host-side group helpers.  Caller records are plain byte buffers without alignment guarantees,
// so every access goes through aligned locals.
template <class F>
static void generic_point_add(void *r, const void *a, const void *b, u64 n) {
  for (u64 i = 0; i < n; i++) {
    Affine<F> pa, pb, pr;
    memcpy(&pa, (const char *)a + i * sizeof pa, sizeof pa);
    memcpy(&pb, (const char *)b + i * sizeof pb, sizeof pb);
    XYZZ<F> x, y, z;
    xyzz_from_affine(x, pa);
    xyzz_from_affine(y, pb);
    xyzz_add(z, x, y);
    xyzz_to_affine(pr, z);
    memcpy((char *)r + i * sizeof pr, &pr, sizeof pr);
  }
}
template <class F>
static void generic_point_mul(void *r, const void *a, const void *k) {
  Affine<F> base, res;
  u32 kw[8];
  memcpy(&base, a, sizeof base);
  memcpy(kw, k, sizeof kw);
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  for (int b = 255; b >= 0; b--) {
    XYZZ<F> t;
    xyzz_dbl(t, acc);
    acc = t;
    if (((kw[b >> 5] >> (b & 31)) & 1) && !aff_is_identity(base)) xyzz_madd(acc, base);
  }
  xyzz_to_affine(res, acc);
  memcpy(r, &res, sizeof res);
}
// [k] a with signed 4-bit windows: 8 precomputed multiples, 256 doublings, at most 64 additions (the plain
// double-and-add above costs ~128 more additions); the serial tails of create_proof (prover.rs:326-354) and the
// tiny-multiexp path run on the host, where this is ~2x faster
template <class F>
static void windowed_point_mul(void *r, const void *a, const u32 *k) {
  Affine<F> base, res;
  memcpy(&base, a, sizeof base);
  u32 kw[9];
  memcpy(kw, k, 32);
  kw[8] = 0;
  bool zero = true;
  for (int i = 0; i < 8; i++) zero &= kw[i] == 0;
  if (aff_is_identity(base) || zero) {
    memset(r, 0, sizeof res);
    return;
  }
  XYZZ<F> tab[8];   // (i + 1) * base
  xyzz_from_affine(tab[0], base);
  xyzz_dbl(tab[1], tab[0]);
  for (int i = 2; i < 8; i++) xyzz_add(tab[i], tab[i - 1], tab[0]);
  // signed digits d_j in [-8, 8], low to high with carry; 65 digits cover a 256-bit scalar + carry
  int digits[65];
  u32 carry = 0;
  for (int j = 0; j < 65; j++) {
    u32 v = (j < 64 ? (kw[j >> 3] >> ((j & 7) * 4)) & 15u : 0u) + carry;
    carry = 0;
    int d = (int)v;
    if (v > 8) { d = (int)v - 16; carry = 1; }
    digits[j] = d;
  }
  XYZZ<F> acc, t;
  xyzz_set_identity(acc);
  for (int j = 64; j >= 0; j--) {
    for (int b = 0; b < 4; b++) { xyzz_dbl(t, acc); acc = t; }
    const int d = digits[j];
    if (d) {
      XYZZ<F> q = tab[(d < 0 ? -d : d) - 1];
      if (d < 0) F::neg(q.y, q.y);
      xyzz_add(t, acc, q);
      acc = t;
    }
  }
  xyzz_to_affine(res, acc);
  memcpy(r, &res, sizeof res);
}
// sum_i [k_i] P_i on the host with ONE doubling chain (Straus, signed 4-bit windows per term) and one final inversion:
// the tail of create_proof folds g_c = ... + [s] a_answer + [r] b1_answer + h + l (prover.rs:339-354) - as separate
// scalar multiplications and affine additions that was two doubling chains and nine inversions.  Scalars equal to one
// cost a single addition.
template <class F>
static void point_lincomb(void *r, const void *pts, const u32 *scalars, u64 n) {
  struct Term {
    XYZZ<F> tab[8];
    int digits[65];
  };
  std::vector<Term> terms;
  std::vector<Affine<F>> ones;
  terms.reserve(n);
  for (u64 i = 0; i < n; i++) {
    Affine<F> base;
    memcpy(&base, (const char *)pts + i * sizeof base, sizeof base);
    u32 kw[9];
    if (scalars) memcpy(kw, scalars + 8 * i, 32); else { memset(kw, 0, 32); kw[0] = 1; }
    kw[8] = 0;
    bool zero = true, one = kw[0] == 1;
    for (int j = 0; j < 8; j++) { zero &= kw[j] == 0; if (j) one &= kw[j] == 0; }
    if (aff_is_identity(base) || zero) continue;
    if (one) { ones.push_back(base); continue; }
    terms.emplace_back();
    Term &t = terms.back();
    xyzz_from_affine(t.tab[0], base);
    xyzz_dbl(t.tab[1], t.tab[0]);
    for (int j = 2; j < 8; j++) xyzz_add(t.tab[j], t.tab[j - 1], t.tab[0]);
    u32 carry = 0;
    for (int j = 0; j < 65; j++) {
      u32 v = (j < 64 ? (kw[j >> 3] >> ((j & 7) * 4)) & 15u : 0u) + carry;
      carry = 0;
      int d = (int)v;
      if (v > 8) { d = (int)v - 16; carry = 1; }
      t.digits[j] = d;
    }
  }
  XYZZ<F> acc, tmp;
  xyzz_set_identity(acc);
  if (!terms.empty()) {
    for (int j = 64; j >= 0; j--) {
      if (!xyzz_is_identity(acc)) for (int b = 0; b < 4; b++) { xyzz_dbl(tmp, acc); acc = tmp; }
      for (Term &t : terms) {
        const int d = t.digits[j];
        if (!d) continue;
        XYZZ<F> q = t.tab[(d < 0 ? -d : d) - 1];
        if (d < 0) F::neg(q.y, q.y);
        xyzz_add(tmp, acc, q);
        acc = tmp;
      }
    }
  }
  for (const Affine<F> &b : ones) xyzz_madd(acc, b);
  Affine<F> res;
  xyzz_to_affine(res, acc);
  memcpy(r, &res, sizeof res);
}
// fast path: 64-bit-limb host arithmetic
template <class FD> static void host_point_lincomb_t(void *r, const void *pts, const u32 *scalars, u64 n) {
  point_lincomb<typename HostOf<FD>::type>(r, pts, scalars, n);
}
template <class FD> static void host_point_add_t(void *r, const void *a, const void *b, u64 n) {
  generic_point_add<typename HostOf<FD>::type>(r, a, b, n);
}
template <class FD> static void host_point_mul_t(void *r, const void *a, const u32 *k) {
  windowed_point_mul<typename HostOf<FD>::type>(r, a, k);
}
// the DEVICE headers compiled for the host (32-bit limbs): CPU-side unit tests of ff.cuh / ec.cuh
template <class F> static void devhdr_point_add_t(void *r, const void *a, const void *b, u64 n) {
  generic_point_add<F>(r, a, b, n);
}
template <class F> static void devhdr_point_mul_t(void *r, const void *a, const u32 *k) { generic_point_mul<F>(r, a, k); }

}  // namespace bh
