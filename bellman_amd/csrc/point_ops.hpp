// What point_fft.hip and point_mul.hip export: EvaluationDomain over vectors of G1 / G2 points, and one scalar
// multiplication per point.
#pragma once
#include "common.hpp"

namespace bh {
// point_fft.hip
int point_fft(Context &c, int group, void *pts, uint32_t log_n, int mode, hipStream_t st);
int point_distribute_powers(Context &c, int group, void *pts, u64 n, const fr_t &g, hipStream_t st);
int point_divide_by_z(int group, void *pts, uint32_t log_n, hipStream_t st);
int point_mul_assign(int group, void *pts, const void *scalars_mont, u64 n, hipStream_t st);
int point_sub_assign(int group, void *a, const void *b, u64 n, hipStream_t st);
// point_mul.hip
int point_mul_each(int group, const void *in, void *out, u64 n, const void *scalars, int fmt, hipStream_t st);
int point_mul_powers(Context &c, int group, const void *in, void *out, u64 n, const fr_t &cc, const fr_t &g, hipStream_t st);
}  // namespace bh
