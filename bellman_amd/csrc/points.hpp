// Reading, validating and combining point records outside a multiexp job: the status word of the loaders, the compressed
// readers (point_read.hip), the curve and subgroup tests, the window-table builders and the host-side group law
// (point_kernels.cuh and msm_ec.cuh, instantiated in msm_g1.hip / msm_g2.hip; the by-group dispatchers are in msm.hip).
#pragma once
#include "msm_types.hpp"

namespace bh {

// per-point status word of the uncompressed-point loader (api_bases.hip decode kernel + point_check_kernel)
enum PointStatus : u32 {
  PT_COMPRESSED = 1,        // compression flag set on an uncompressed point
  PT_SORT = 2,              // sort flag set on an uncompressed point
  PT_RANGE = 4,             // a coordinate is not < p
  PT_INF_NONZERO = 8,       // infinity flag with non-zero coordinate bits
  PT_IS_INF = 16,           // (valid) identity
  PT_OFF_CURVE = 32,
  PT_NOT_IN_SUBGROUP = 64,
  PT_NOT_COMPRESSED = 128,  // compression flag clear on a compressed point (set by the compressed reader only)
  PT_INVALID_MASK = PT_COMPRESSED | PT_SORT | PT_RANGE | PT_INF_NONZERO | PT_OFF_CURVE | PT_NOT_IN_SUBGROUP | PT_NOT_COMPRESSED,
};
// The compressed reader (point_read.hip) uses the same word: PT_SORT = sort flag on an infinity encoding, PT_OFF_CURVE =
// x^3 + b is not a square (no point has this x).  Where lane i of its kernel finds its point, its record and its status
// word: group g = i / per, element e = i % per; byte offsets g * stride + first + e * step (status: in words).
struct ReadLayout {
  size_t in_stride, in_first, in_step;
  size_t out_stride, out_first, out_step;
  u32 per;
  u32 st_stride, st_first, st_step;
};
int points_read_compressed(int group, const void *raw_dev, void *out_dev, u64 n, const ReadLayout &lay, bool checked,
                           u32 *status_dev, hipStream_t st);
// status words (PT_IS_INF; with `checked` PT_RANGE, PT_OFF_CURVE, PT_NOT_IN_SUBGROUP) of n resident affine records
int points_validate(int group, const void *pts_dev, u64 n, bool checked, u32 *status_dev, hipStream_t st);
int proofs_read_dev(const void *bytes_dev, void *proofs_out_dev, u64 n, u32 *pst, u32 *words, unsigned long long *min_idx,
                    hipStream_t st);
// the error a sequential reader reports for a proof with this status word: the first bad element in the order a, b, c
inline int proof_status_error(u32 word) {
  for (int k = 0; k < 3; k++) {
    const u32 s = (word >> (8 * k)) & 0xffu;
    if (s & PT_INVALID_MASK) return BH_ERR_INVALID_POINT;
    if (s & PT_IS_INF) return BH_ERR_POINT_AT_INFINITY;
  }
  return BH_OK;
}
// writes the W rows of a window table over the n records of `src` at their final place: row j record i at
// dst + (j * n + i) * dst_stride bytes (dst_stride >= the record size; bytes between records are left as they are)
int window_table_g1(BaseView src, void *dst, u32 dst_stride, u64 n, u32 c, u32 W, hipStream_t st);
int window_table_g2(BaseView src, void *dst, u32 dst_stride, u64 n, u32 c, u32 W, hipStream_t st);
int window_table(int group, BaseView src, void *dst, u32 dst_stride, u64 n, u32 c, u32 W, hipStream_t st);
// on-curve + prime-order-subgroup test of decoded points (skips entries already invalid / identity)
int points_check_g1(const void *pts_dev, u64 n, u32 *status_dev, hipStream_t st);
int points_check_g2(const void *pts_dev, u64 n, u32 *status_dev, hipStream_t st);
int points_check(int group, const void *pts_dev, u64 n, u32 *status_dev, hipStream_t st);
void host_point_add_g1(void *r, const void *a, const void *b, u64 n);
void host_point_add_g2(void *r, const void *a, const void *b, u64 n);
void host_point_mul_g1(void *r, const void *a, const void *k);
void host_point_mul_g2(void *r, const void *a, const void *k);
void host_point_lincomb_g1(void *r, const void *pts, const void *scalars, u64 n);
void host_point_lincomb_g2(void *r, const void *pts, const void *scalars, u64 n);
void host_point_add(int group, void *r, const void *a, const void *b, u64 n);
void host_point_mul(int group, void *r, const void *a, const void *k);
void host_point_lincomb(int group, void *r, const void *pts, const void *scalars, u64 n);

}  // namespace bh
