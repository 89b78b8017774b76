// What fft.hip exports to the other units of the library: the Fr transforms and element-wise passes behind
// EvaluationDomain, and the power tables and domain constants the point transforms share with them.
#pragma once
#include "common.hpp"

namespace bh {
int ntt_run(Context &c, fr_t *data, fr_t *scratch, uint32_t log_n, int mode, hipStream_t st);
int fr_mul_assign(Context &c, fr_t *a, const fr_t *b, u64 n, hipStream_t st);
int fr_sub_assign(Context &c, fr_t *a, const fr_t *b, u64 n, hipStream_t st);
int fr_divide_by_z(Context &c, fr_t *a, uint32_t log_n, hipStream_t st);
int fr_distribute_powers(Context &c, fr_t *a, u64 n, const fr_t &g, hipStream_t st);
int h_poly_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, fr_t *scratch, uint32_t log_n, hipStream_t st);
int fr_gen_powers(Context &c, fr_t *out, u64 n, const fr_t &g, const fr_t &scale, hipStream_t st);
int ntt_run_many(Context &c, fr_t *data, u64 stride, u64 k, uint32_t log_n, int mode, fr_t *scratch, u64 scratch_vectors, hipStream_t st);
int ntt_run_each(Context &c, fr_t *data, u64 stride, u64 k, uint32_t log_n, int mode, fr_t *scratch, hipStream_t st);
int h_poly_many_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, u64 stride, u64 k, uint32_t log_n, fr_t *scratch, u64 scratch_vectors,
                    hipStream_t st);
int h_poly_each_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, u64 stride, u64 k, uint32_t log_n, fr_t *scratch, hipStream_t st);
// the Fr power tables and domain constants shared with the point transforms (point_fft.hip, point_mul.hip)
int launch_gen_powers(fr_t *out, u64 n, const fr_t &g, const fr_t &scale, int mul_into, hipStream_t st);
fr_t fr_domain_omega_host(uint32_t log_n);
fr_t fr_from_u64_host(u64 v);
fr_t zinv_host(uint32_t log_n);
// the context's table cache (bh_ctx_trim, bh_ctx_destroy)
void fft_tables_free(FftTables &t);
void fft_master_free(Context &c);
}  // namespace bh
