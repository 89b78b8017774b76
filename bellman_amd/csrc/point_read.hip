// from_compressed / from_compressed_unchecked of bls12_381 on the device: the compressed Zcash encoding (48 bytes for G1,
// 96 for G2: x big-endian, G2 c1 before c0, the flag bits compressed / infinity / sort in the top of byte 0) -> affine
// Montgomery records plus a PointStatus word per point.  What Proof::read (groth16/src/lib.rs:47-99) does to the three
// points of a proof; declared in points.hpp, called from api_bases.hip (bh_bases_read_compressed) and pairing.hip
// (bh_proofs_read, bh_groth16_batch_verify_compressed).
//
// One lane per point:
//   1. decode: flag bits, x < p (every coordinate), a clean infinity encoding; x to Montgomery form
//   2. y = sqrt(x^3 + b) (point_read.cuh), the root whose "lexicographically largest" equals the sort flag
//   3. (checked) subgroup membership by endomorphism instead of [q] P:
//        G1  (beta x, y) == -[|z|] [|z|] P    two multiplications by the 64-bit |z| (Hamming weight 6)
//        G2  psi(P) == -[|z|] P               one
//      compared in XYZZ form without an inversion
//   4. the affine record (all-zero for the identity and for every invalid point) and the status word
// A lane whose point is already invalid or the identity takes no part in steps 2 and 3 (its lanes are masked off; the
// loops are over compile-time constants and the same for every lane).
#include "common.hpp"
#include "point_read.cuh"
#include "points.hpp"

namespace bh {

// ---- per-field pieces ---------------------------------------------------------------------------------------------------
// 48 big-endian bytes -> little-endian limbs (the three flag bits still in place)
__device__ __forceinline__ void load_be48(fp_t &v, const u32 *src) {
#pragma unroll
  for (int w = 0; w < 12; w++) v.l[w] = __builtin_bswap32(src[11 - w]);
}
__device__ __forceinline__ bool fp_in_range(const fp_t &v) {   // canonical coordinate: value < p
  u32 br = 0;
#pragma unroll
  for (int w = 0; w < 12; w++) (void)subb(v.l[w], FpParams::mod(w), br, br);
  return br != 0;
}
// x as written (flags stripped, NOT Montgomery); returns the flag bits (4 compressed, 2 infinity, 1 sort)
__device__ __forceinline__ u32 load_x(fp_t &x, const u32 *src, bool &in_range, bool &nonzero) {
  load_be48(x, src);
  const u32 flags = x.l[11] >> 29;
  x.l[11] &= 0x1fffffffu;
  in_range = fp_in_range(x);
  nonzero = !fe_is_zero(x);
  return flags;
}
__device__ __forceinline__ u32 load_x(fp2_t &x, const u32 *src, bool &in_range, bool &nonzero) {
  load_be48(x.c1, src);   // c1 travels first and carries the flags
  load_be48(x.c0, src + 12);
  const u32 flags = x.c1.l[11] >> 29;
  x.c1.l[11] &= 0x1fffffffu;
  in_range = fp_in_range(x.c0) && fp_in_range(x.c1);
  nonzero = !(fe_is_zero(x.c0) && fe_is_zero(x.c1));
  return flags;
}
__device__ __forceinline__ void x_to_mont(fp_t &x) { fe_to_mont(x, x); }
__device__ __forceinline__ void x_to_mont(fp2_t &x) {
  fe_to_mont(x.c0, x.c0);
  fe_to_mont(x.c1, x.c1);
}
__device__ __forceinline__ bool field_sqrt(fp_t &r, const fp_t &a) { return fp_sqrt(r, a); }
__device__ __forceinline__ bool field_sqrt(fp2_t &r, const fp2_t &a) { return fp2_sqrt(r, a); }
__device__ __forceinline__ bool lex_largest(const fp_t &y) { return fp_lex_largest(y); }
__device__ __forceinline__ bool lex_largest(const fp2_t &y) { return fp2_lex_largest(y); }
__device__ __forceinline__ void neg_canonical(fp_t &y) { fe_neg(y, y); }
__device__ __forceinline__ void neg_canonical(fp2_t &y) {
  fe_neg(y.c0, y.c0);
  fe_neg(y.c1, y.c1);
}

// acc = [|z|] base: 63 doublings and 5 additions, the bits of |z| being compile-time constants
template <class F>
__device__ __forceinline__ void mul_z(XYZZ<F> &acc, const Affine<F> &base) {
  xyzz_from_affine(acc, base);
  for (int bit = 62; bit >= 0; bit--) {
    XYZZ<F> t;
    xyzz_dbl(t, acc);
    acc = t;
    if ((BLS_Z_ABS >> bit) & 1) xyzz_madd(acc, base);
  }
}
template <class F>
__device__ __forceinline__ void mul_z(XYZZ<F> &acc, const XYZZ<F> &base) {
  acc = base;
  for (int bit = 62; bit >= 0; bit--) {
    XYZZ<F> t;
    xyzz_dbl(t, acc);
    acc = t;
    if ((BLS_Z_ABS >> bit) & 1) xyzz_add(acc, acc, base);
  }
}
// the affine point (ex, ey) equals -q
template <class F>
__device__ __forceinline__ bool equals_neg(const typename F::T &ex, const typename F::T &ey, const XYZZ<F> &q) {
  if (xyzz_is_identity(q)) return false;
  typename F::T t;
  F::mul(t, ex, q.zz);
  if (!F::eq(t, q.x)) return false;
  F::mul(t, ey, q.zzz);
  F::add(t, t, q.y);
  return F::is_zero(t);
}
// P (valid, not the identity) is in the prime-order subgroup
// (`slot`: the lane's place in LDS.  P and [|z|] P - the bases of the two multiplications, needed only at their five
// additions each - wait there instead of occupying 24 + 48 registers next to the accumulator and the temporaries of the
// general addition: that is what lets two wavefronts share a SIMD without spilling)
struct G1Slot {
  Affine<FpOps> p;
  XYZZ<FpOps> q;
};
__device__ __forceinline__ bool in_subgroup(const Affine<FpOps> &p, G1Slot &slot) {
  XYZZ<FpOps> acc;
  slot.p = p;
  mul_z(acc, slot.p);
  slot.q = acc;
  mul_z(acc, slot.q);   // [z^2] P
  fp_t beta, ex;
#pragma unroll
  for (int i = 0; i < 12; i++) beta.l[i] = EndoConsts::beta(i);
  FpOps::mul(ex, slot.p.x, beta);
  return equals_neg<FpOps>(ex, slot.p.y, acc);
}
__device__ __forceinline__ bool in_subgroup(const Affine<Fp2Ops> &p, G1Slot &) {
  XYZZ<Fp2Ops> q;
  mul_z(q, p);       // [|z|] P = -[z] P
  fp2_t cx, cy, ex, ey;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    cx.c0.l[i] = EndoConsts::psi_cx(i);
    cx.c1.l[i] = EndoConsts::psi_cx(12 + i);
    cy.c0.l[i] = EndoConsts::psi_cy(i);
    cy.c1.l[i] = EndoConsts::psi_cy(12 + i);
  }
  ex = p.x;
  ey = p.y;
  fpl_neg(ex.c1, ex.c1);   // the conjugates
  fpl_neg(ey.c1, ey.c1);
  Fp2Ops::mul(ex, ex, cx);
  Fp2Ops::mul(ey, ey, cy);
  return equals_neg<Fp2Ops>(ex, ey, q);
}

// every coordinate of a resident record is a canonical value (< p)
__device__ __forceinline__ bool coords_in_range(const Affine<FpOps> &p) { return fp_in_range(p.x) && fp_in_range(p.y); }
__device__ __forceinline__ bool coords_in_range(const Affine<Fp2Ops> &p) {
  return fp_in_range(p.x.c0) && fp_in_range(p.x.c1) && fp_in_range(p.y.c0) && fp_in_range(p.y.c1);
}

// ---- the kernel --------------------------------------------------------------------------------------------------------
// Lane i reads point e = i % per of group g = i / per: the `per` points of one group (a proof's A and C; 1 for a plain
// vector) sit in_step / out_step / st_step apart, groups in_stride / out_stride / st_stride apart.  Offsets in bytes
// (status: words); every point starts on a 4-byte boundary.
template <class F>
__global__ void __launch_bounds__(64, F::WORDS == 12 ? 2 : 1)
    read_compressed_kernel(const unsigned char *raw, unsigned char *out, ReadLayout lay, u64 n, u32 checked, u32 *status) {
  typedef typename F::T T;
  __shared__ G1Slot slots[F::WORDS == 12 ? 64 : 1];   // G1 only, see in_subgroup
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 g = i / lay.per, e = i - g * lay.per;
  const u32 *src = reinterpret_cast<const u32 *>(raw + g * lay.in_stride + lay.in_first + e * lay.in_step);
  T x;
  bool in_range, nonzero;
  const u32 flags = load_x(x, src, in_range, nonzero);
  u32 st = 0;
  if (!(flags & 4u)) st |= PT_NOT_COMPRESSED;
  if (!in_range) st |= PT_RANGE;
  if (flags & 2u) {   // the identity: nothing else may be set
    st |= PT_IS_INF;
    if (flags & 1u) st |= PT_SORT;
    if (nonzero) st |= PT_INF_NONZERO;
  }
  Affine<F> *rec = reinterpret_cast<Affine<F> *>(out + g * lay.out_stride + lay.out_first + e * lay.out_step);
  bool keep = false;   // the record written below stands
  if (!(st & (PT_INVALID_MASK | PT_IS_INF))) {
    x_to_mont(x);
    T rhs, b, y;
    F::sqr(rhs, x);
    F::mul(rhs, rhs, x);
    F::curve_b(b);
    F::add(rhs, rhs, b);
    if (!field_sqrt(y, rhs)) {
      st |= PT_OFF_CURVE;   // x^3 + b is not a square: no point of the curve has this x
    } else {
      F::canon(y);
      if (lex_largest(y) != ((flags & 1u) != 0)) neg_canonical(y);   // (y != 0: both curve orders are odd)
      Affine<F> p;
      p.x = x;
      p.y = y;
      *rec = p;   // before the subgroup test, so that it need not stay in registers through it
      keep = !checked || in_subgroup(p, slots[F::WORDS == 12 ? threadIdx.x : 0]);
      if (!keep) st |= PT_NOT_IN_SUBGROUP;
    }
  }
  if (!keep) {   // the identity and every invalid point: the all-zero record
    Affine<F> zero;
    F::zero(zero.x);
    F::zero(zero.y);
    *rec = zero;
  }
  status[g * lay.st_stride + lay.st_first + e * lay.st_step] = st;
}

// ---- validation of records already resident (bh_bases_validate) --------------------------------------------------------
// One lane per affine Montgomery record: the identity (the all-zero record) is PT_IS_INF; with `checked` every other record
// must hold coordinates < p (PT_RANGE), satisfy y^2 = x^3 + b (PT_OFF_CURVE) and pass the endomorphism subgroup test above
// (PT_NOT_IN_SUBGROUP).  Same launch bounds and LDS parking as the compressed reader; a lane whose record is the identity
// or already invalid is masked off during the multiplications.  Nothing is written but the status word.
template <class F>
__global__ void __launch_bounds__(64, F::WORDS == 12 ? 2 : 1)
    validate_kernel(const Affine<F> *pts, u64 n, u32 checked, u32 *status) {
  __shared__ G1Slot slots[F::WORDS == 12 ? 64 : 1];   // G1 only, see in_subgroup
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = pts[i];
  u32 st = 0;
  if (aff_is_identity(p)) {
    st = PT_IS_INF;
  } else if (checked) {
    if (!coords_in_range(p)) st = PT_RANGE;
    else if (!on_curve(p)) st = PT_OFF_CURVE;
    else if (!in_subgroup(p, slots[F::WORDS == 12 ? threadIdx.x : 0])) st = PT_NOT_IN_SUBGROUP;
  }
  status[i] = st;
}

int points_validate(int group, const void *pts_dev, u64 n, bool checked, u32 *status_dev, hipStream_t st) {
  if (!n) return BH_OK;
  const u32 blocks = (u32)((n + 63) / 64);
  (void)hipGetLastError();
  if (group == BH_G1)
    hipLaunchKernelGGL(validate_kernel<FpOps>, dim3(blocks), dim3(64), 0, st, (const Affine<FpOps> *)pts_dev, n,
                       checked ? 1u : 0u, status_dev);
  else
    hipLaunchKernelGGL(validate_kernel<Fp2Ops>, dim3(blocks), dim3(64), 0, st, (const Affine<Fp2Ops> *)pts_dev, n,
                       checked ? 1u : 0u, status_dev);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// a proof's status word from the PointStatus bits of its three points (a | b << 8 | c << 16), and the first bad proof
__global__ void proof_status_kernel(const u32 *pst, u64 n, u32 *words, unsigned long long *min_idx) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const u32 w = (pst[3 * i] & 0xffu) | ((pst[3 * i + 1] & 0xffu) << 8) | ((pst[3 * i + 2] & 0xffu) << 16);
    words[i] = w;
    if (w) atomicMin(min_idx, (unsigned long long)i);
  }
}

int points_read_compressed(int group, const void *raw_dev, void *out_dev, u64 n, const ReadLayout &lay, bool checked,
                           u32 *status_dev, hipStream_t st) {
  if (!n) return BH_OK;
  const u32 blocks = (u32)((n + 63) / 64);
  (void)hipGetLastError();
  if (group == BH_G1)
    hipLaunchKernelGGL(read_compressed_kernel<FpOps>, dim3(blocks), dim3(64), 0, st, (const unsigned char *)raw_dev,
                       (unsigned char *)out_dev, lay, n, checked ? 1u : 0u, status_dev);
  else
    hipLaunchKernelGGL(read_compressed_kernel<Fp2Ops>, dim3(blocks), dim3(64), 0, st, (const unsigned char *)raw_dev,
                       (unsigned char *)out_dev, lay, n, checked ? 1u : 0u, status_dev);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// Proof::read of n proofs already on the device: 192-byte A | B | C -> 384-byte affine a | b | c.  pst: 3 n words of
// workspace, words: n status words, min_idx: set to the first proof with a non-zero word (untouched when there is none)
int proofs_read_dev(const void *bytes_dev, void *proofs_out_dev, u64 n, u32 *pst, u32 *words, unsigned long long *min_idx,
                    hipStream_t st) {
  if (!n) return BH_OK;
  const ReadLayout g1 = {192, 0, 144, 384, 0, 288, 2, 3, 0, 2};   // A and C of every proof
  const ReadLayout g2 = {192, 48, 0, 384, 96, 0, 1, 3, 1, 0};     // B
  int rc = points_read_compressed(BH_G2, bytes_dev, proofs_out_dev, n, g2, true, pst, st);
  if (rc == BH_OK) rc = points_read_compressed(BH_G1, bytes_dev, proofs_out_dev, 2 * n, g1, true, pst, st);
  if (rc != BH_OK) return rc;
  const u64 blocks = (n + 255) / 256;
  hipLaunchKernelGGL(proof_status_kernel, dim3((u32)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, pst, n, words, min_idx);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // namespace bh
