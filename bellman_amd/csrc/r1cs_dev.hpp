// The device-resident R1CS handle (bh_r1cs), shared by r1cs.hip (products with Fr vectors) and r1cs_points.hip
// (products with vectors of group elements).
#pragma once
#include <mutex>
#include <vector>

#include "common.hpp"

// A row with more terms than this is summed by a whole workgroup instead of one lane: the constant
// ONE typically appears in every constraint, so its row of a transposed matrix has ~n terms.
namespace bh {
constexpr u32 LONG_ROW = 1024;
// Witnesses per lane of the k-witness kernels (r1cs.hip: r1cs_eval_many_kernel, r1cs_check_many_kernel): a lane reads a term
// record and its coefficient once and applies them to this many witnesses.  The largest of 2, 4, 8 at which clang reports no
// scratch and at most 128 VGPRs for every one of those kernels (tools/kernel_resources.py r1cs.hip; the line is in DESIGN.md
// 5.4.1): the kernels are bound by the latency of the witness gathers and want waves in flight.
constexpr u32 R1CS_MANY_TILE = 2;
}

struct bh_r1cs {
  bh_ctx *ctx = nullptr;
  size_t n_inputs = 0, n_aux = 0, n_constraints = 0, n_coeffs = 0;
  bh::u32 *row_ptr[3] = {nullptr, nullptr, nullptr};    // [n_constraints + 1]
  uint2 *terms[3] = {nullptr, nullptr, nullptr};    // (variable, coefficient index)
  bh::fr_t *coeffs = nullptr;                           // Montgomery; index 0 is always 1
  bh::u64 *dens[3] = {nullptr, nullptr, nullptr};       // a_aux, b_input, b_aux (LSB0 words, device)
  size_t dens_total[3] = {0, 0, 0};
  std::vector<bh::u64> dens_host[3];
  // host copy of the matrices + the transposed (variable-major) device copy the parameter generator
  // uses (generator.rs:43-131 stores exactly that: per variable, (coeff, constraint) lists); built on
  // first use
  uint2 *long_rows = nullptr;                        // (matrix, row) of rows with more than LONG_ROW terms
  bh::u32 n_long = 0;
  uint2 *t_long_rows = nullptr;                      // the same for the transposed matrices
  bh::u32 t_n_long = 0;
  bh::u32 *long_cons = nullptr;                      // constraints with more than LONG_ROW terms in their A, B or C row
  bh::u32 n_long_cons = 0;
  std::vector<bh::u32> h_row_ptr[3], h_var[3], h_coeff[3];
  std::mutex t_mu;
  bool t_ready = false;
  bh::u32 *t_row_ptr[3] = {nullptr, nullptr, nullptr};   // [n_inputs + n_aux + 1]
  uint2 *t_terms[3] = {nullptr, nullptr, nullptr};   // (constraint, coefficient index)
  // The plan of the group-valued transposed product (r1cs_points.hip), built on its first use under t_mu:
  //   coeff_canon / coeff_info   per coefficient-table entry: canonical form, class and bit length
  //   p_terms[m]                 the transposed terms once more as (constraint, code): code 0 adds the Lagrange point, 1
  //                              subtracts it, 2 is a zero coefficient, code >= 3 adds entry code - 3 of the scaled pool
  //   gen_terms[m]               indices into t_terms[m] of the terms with a general coefficient, longest coefficient
  //                              first; entry g of the scaled pool is [coefficient] Lagrange point of term gen_terms[m][g]
  bool p_ready = false;
  bh::fr_t *coeff_canon = nullptr;
  bh::u32 *coeff_info = nullptr;
  uint2 *p_terms[3] = {nullptr, nullptr, nullptr};
  bh::u32 *gen_terms[3] = {nullptr, nullptr, nullptr};
  bh::u32 n_gen[3] = {0, 0, 0};
  std::vector<uint2> h_t_terms[3];                   // host copy of t_terms, dropped once the plan exists
};

namespace bh {
// builds t_row_ptr / t_terms / t_long_rows on first use (r1cs.hip)
int r1cs_ensure_transposed(bh_ctx *ctx, bh_r1cs *r);
template <class T>
int r1cs_upload_vec(bh_ctx *ctx, T **dst, const T *src, size_t n) {
  *dst = (T *)ctx->c.pool.acquire((n ? n : 1) * sizeof(T));
  if (!*dst) return BH_ERR_HIP;
  if (n) BH_HIP_CHECK(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->c.stream));
  return BH_OK;
}
}  // namespace bh
