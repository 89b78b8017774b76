// R1CS matrices resident in HBM + the evaluation of all constraints' linear combinations on the
// device.  The reference evaluates the three LinearCombinations of every
// constraint on one host thread while the circuit is synthesised
// (/root/reference/groth16/src/prover.rs:19-55 `eval`, :105-145 `enforce`).  The matrices do not
// depend on the witness, so they are captured once per circuit (like the CRS) and a proof only needs
//   a[i] = <A_i, w>,  b[i] = <B_i, w>,  c[i] = <C_i, w>      (w = input_assignment | aux_assignment)
// which is one sparse matrix-vector product per matrix: one lane per (matrix, constraint) row.
// The query densities (prover.rs:31-44: a variable counts only through a non-zero coefficient) are a
// function of the matrices alone and are computed here once.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "r1cs_dev.hpp"

using namespace bh;

namespace {

struct R1csEvalArgs {
  const u32 *row_ptr[3];
  const uint2 *terms[3];
  fr_t *out[3];
  const fr_t *coeffs, *inputs, *aux;
  u32 n_inputs;
  u64 n_constraints, m;   // rows >= n_constraints are the zero padding of from_coeffs (domain.rs:68)
  const uint2 *long_rows; // rows the lane-per-row kernel leaves to r1cs_long_rows_kernel
};

__global__ void __launch_bounds__(256) r1cs_eval_kernel(R1csEvalArgs a) {
  const u64 total = 3 * a.m;
  for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (u64)gridDim.x * blockDim.x) {
    const u32 mat = (u32)(g / a.m);
    const u64 row = g - (u64)mat * a.m;
    fr_t acc;
    fe_zero(acc);
    if (row < a.n_constraints) {
      const u32 lo = a.row_ptr[mat][row], hi = a.row_ptr[mat][row + 1];
      if (hi - lo > LONG_ROW) continue;   // written by r1cs_long_rows_kernel
      for (u32 t = lo; t < hi; t++) {
        const uint2 term = a.terms[mat][t];
        fr_t w = ld_fr16(term.x < a.n_inputs ? a.inputs + term.x : a.aux + (term.x - a.n_inputs));
        if (term.y != 0) {           // coefficient 1 is by far the most common one (prover.rs:47-52)
          const fr_t k = ld_fr16(a.coeffs + term.y);
          fe_mul(w, w, k);
        }
        fe_add(acc, acc, w);
      }
    }
    st_fr16(a.out[mat] + row, acc);
  }
}

__global__ void __launch_bounds__(256) qap_ext_kernel(fr_t *e, const fr_t *at, const fr_t *bt, const fr_t *ct, u64 n_inputs,
                                                      u64 n, fr_t alpha, fr_t beta, fr_t gamma_inv, fr_t delta_inv) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    fr_t a = ld_fr16(at + i), b = ld_fr16(bt + i), c = ld_fr16(ct + i);
    fe_mul(a, a, beta);
    fe_mul(b, b, alpha);
    fe_add(a, a, b);
    fe_add(a, a, c);
    if (i < n_inputs) fe_mul(a, a, gamma_inv); else fe_mul(a, a, delta_inv);
    st_fr16(e + i, a);
  }
}

__global__ void __launch_bounds__(256) r1cs_long_rows_kernel(R1csEvalArgs a) {
  __shared__ fr_t part[256];
  const uint2 job = a.long_rows[blockIdx.x];
  const u32 mat = job.x, row = job.y;
  const u32 lo = a.row_ptr[mat][row], hi = a.row_ptr[mat][row + 1];
  fr_t acc;
  fe_zero(acc);
  for (u32 t = lo + threadIdx.x; t < hi; t += 256) {
    const uint2 term = a.terms[mat][t];
    fr_t w = ld_fr16(term.x < a.n_inputs ? a.inputs + term.x : a.aux + (term.x - a.n_inputs));
    if (term.y != 0) {
      const fr_t k = ld_fr16(a.coeffs + term.y);
      fe_mul(w, w, k);
    }
    fe_add(acc, acc, w);
  }
  part[threadIdx.x] = acc;
  for (u32 off = 128; off >= 1; off >>= 1) {
    __syncthreads();
    if (threadIdx.x < off) {
      fr_t x = part[threadIdx.x], y = part[threadIdx.x + off];
      fe_add(x, x, y);
      part[threadIdx.x] = x;
    }
  }
  if (threadIdx.x == 0) st_fr16(a.out[mat] + row, part[0]);
}

// ---- k witnesses against one set of matrices ------------------------------------------------------------------------------
// The matrices do not depend on the witness, so a lane that owns a row reads every term record and every coefficient ONCE
// for a tile of T = R1CS_MANY_TILE witnesses and keeps T accumulators; the tiles over k are the grid's second dimension.
// Witness j is inputs + j * in_stride, aux + j * aux_stride (bytes), output vector j of a matrix out[mat] + j * out_stride.
struct R1csManyArgs {
  const u32 *row_ptr[3];
  const uint2 *terms[3];
  char *out[3];
  const fr_t *coeffs;
  const char *inputs, *aux;
  u64 in_stride, aux_stride, out_stride;
  u32 n_inputs, k;
  u64 n_constraints, m;
  const uint2 *long_rows;   // eval: (matrix, row) of the rows left to r1cs_long_rows_many_kernel
  const u32 *long_cons;     // check: the constraints left to r1cs_check_long_many_kernel
  u32 *first_bad;           // check: one word per witness, BH_R1CS_SATISFIED before the launch
};

// The witnesses of one tile as wave-uniform base pointers.  A ragged last tile repeats its last witness in the slots at and
// beyond n: those slots are computed and never stored or reported, and the term loop needs no branch on the slot.
template <u32 T>
struct TileWitness {
  const fr_t *in[T], *aux[T];
  u32 first, n;
  __device__ __forceinline__ TileWitness(const R1csManyArgs &a, u32 tile) {
    first = tile * T;
    n = a.k - first < T ? a.k - first : T;
#pragma unroll
    for (u32 i = 0; i < T; i++) {
      const u64 j = first + (i < n ? i : n - 1);
      in[i] = reinterpret_cast<const fr_t *>(a.inputs + j * a.in_stride);
      aux[i] = reinterpret_cast<const fr_t *>(a.aux + j * a.aux_stride);
    }
  }
};

// acc[i] += sum over the terms lo, lo + step, ... < hi of one row of coefficient * witness i's variable
template <u32 T>
__device__ __forceinline__ void row_terms_many(fr_t (&acc)[T], const R1csManyArgs &a, const TileWitness<T> &w, u32 mat, u32 lo,
                                               u32 hi, u32 step) {
  for (u32 t = lo; t < hi; t += step) {
    const uint2 term = a.terms[mat][t];
    const bool is_input = term.x < a.n_inputs;
    const u32 idx = is_input ? term.x : term.x - a.n_inputs;
    fr_t c;
    if (term.y != 0) c = ld_fr16(a.coeffs + term.y);   // coefficient 1 is by far the most common one (prover.rs:47-52)
#pragma unroll
    for (u32 i = 0; i < T; i++) {
      fr_t v = ld_fr16((is_input ? w.in[i] : w.aux[i]) + idx);
      if (term.y != 0) fe_mul(v, v, c);
      fe_add(acc[i], acc[i], v);
    }
  }
}

template <u32 T>
__device__ __forceinline__ void zero_many(fr_t (&acc)[T]) {
#pragma unroll
  for (u32 i = 0; i < T; i++) fe_zero(acc[i]);
}

// acc[i] <- the sum of acc[i] over the 256 lanes of the workgroup, in every lane
template <u32 T>
__device__ __forceinline__ void block_sum_many(fr_t (&acc)[T], fr_t *part) {
#pragma unroll
  for (u32 i = 0; i < T; i++) {
    __syncthreads();   // the readers of the slot before are done with part[0]
    part[threadIdx.x] = acc[i];
    for (u32 off = 128; off >= 1; off >>= 1) {
      __syncthreads();
      if (threadIdx.x < off) {
        fr_t x = part[threadIdx.x], y = part[threadIdx.x + off];
        fe_add(x, x, y);
        part[threadIdx.x] = x;
      }
    }
    __syncthreads();
    acc[i] = part[0];
  }
}

template <u32 T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) r1cs_eval_many_kernel(R1csManyArgs a) {
  const TileWitness<T> w(a, blockIdx.y);
  const u64 total = 3 * a.m;
  for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (u64)gridDim.x * blockDim.x) {
    const u32 mat = (u32)(g / a.m);
    const u64 row = g - (u64)mat * a.m;
    fr_t acc[T];
    zero_many(acc);
    if (row < a.n_constraints) {
      const u32 lo = a.row_ptr[mat][row], hi = a.row_ptr[mat][row + 1];
      if (hi - lo > LONG_ROW) continue;   // written by r1cs_long_rows_many_kernel
      row_terms_many(acc, a, w, mat, lo, hi, 1);
    }
#pragma unroll
    for (u32 i = 0; i < T; i++)
      if (i < w.n) st_fr16(reinterpret_cast<fr_t *>(a.out[mat] + (u64)(w.first + i) * a.out_stride) + row, acc[i]);
  }
}

// one workgroup per (long row, tile of witnesses)
template <u32 T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) r1cs_long_rows_many_kernel(R1csManyArgs a) {
  __shared__ fr_t part[256];
  const TileWitness<T> w(a, blockIdx.y);
  const uint2 job = a.long_rows[blockIdx.x];
  const u32 mat = job.x, row = job.y;
  fr_t acc[T];
  zero_many(acc);
  row_terms_many(acc, a, w, mat, a.row_ptr[mat][row] + threadIdx.x, a.row_ptr[mat][row + 1], 256);
  block_sum_many(acc, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (u32 i = 0; i < T; i++)
      if (i < w.n) st_fr16(reinterpret_cast<fr_t *>(a.out[mat] + (u64)(w.first + i) * a.out_stride) + row, acc[i]);
  }
}

// The check, fused: a lane owns one CONSTRAINT and a tile of witnesses, forms <A_i, w> <B_i, w> and <C_i, w> and compares
// them as field elements (both sides are reduced Montgomery forms: equal values are equal words); nothing but first_bad is
// written.  A lane keeps the smallest failing row per witness; the wave takes the minimum over its lanes and issues ONE
// atomicMin per wave and witness - a minimum, so the result does not depend on the order of arrival.
template <u32 T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) r1cs_check_many_kernel(R1csManyArgs a) {
  __shared__ fr_t keep[T][256];
  const TileWitness<T> w(a, blockIdx.y);
  u32 bad[T];
#pragma unroll
  for (u32 i = 0; i < T; i++) bad[i] = BH_R1CS_SATISFIED;
  // (a constraint with a long part is judged by r1cs_check_long_many_kernel; the lane meets the long part when it comes to it
  // and drops the constraint there - the row bounds of the parts behind it need not stay in registers for the test)
  // Only ONE set of T accumulators is in registers at a time: a, and then a * b, wait in the lane's own LDS slots while the
  // next part is summed (no other lane touches them: no barrier) - with two sets in registers the kernel does not fit 128.
  for (u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x; row < a.n_constraints; row += (u64)gridDim.x * blockDim.x) {
    fr_t x[T];
    u32 lo = a.row_ptr[0][row], hi = a.row_ptr[0][row + 1];
    if (hi - lo > LONG_ROW) continue;
    zero_many(x);
    row_terms_many(x, a, w, 0, lo, hi, 1);
#pragma unroll
    for (u32 i = 0; i < T; i++) keep[i][threadIdx.x] = x[i];
    lo = a.row_ptr[1][row]; hi = a.row_ptr[1][row + 1];
    if (hi - lo > LONG_ROW) continue;
    zero_many(x);
    row_terms_many(x, a, w, 1, lo, hi, 1);
#pragma unroll
    for (u32 i = 0; i < T; i++) {
      fr_t p = keep[i][threadIdx.x];
      fe_mul(p, p, x[i]);
      keep[i][threadIdx.x] = p;
    }
    lo = a.row_ptr[2][row]; hi = a.row_ptr[2][row + 1];
    if (hi - lo > LONG_ROW) continue;
    zero_many(x);
    row_terms_many(x, a, w, 2, lo, hi, 1);
#pragma unroll
    for (u32 i = 0; i < T; i++) {
      const fr_t p = keep[i][threadIdx.x];
      if (!fe_eq(p, x[i]) && (u32)row < bad[i]) bad[i] = (u32)row;
    }
  }
#pragma unroll
  for (u32 i = 0; i < T; i++) {
    u32 v = bad[i];
    for (u32 off = 32; off >= 1; off >>= 1) {
      const u32 o = __shfl_xor(v, off);
      v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && i < w.n && v != BH_R1CS_SATISFIED) atomicMin(a.first_bad + w.first + i, v);
  }
}

// one workgroup per (constraint with a long A, B or C row, tile of witnesses): the three parts block-summed, then the compare
template <u32 T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) r1cs_check_long_many_kernel(R1csManyArgs a) {
  __shared__ fr_t part[256];
  const TileWitness<T> w(a, blockIdx.y);
  const u32 row = a.long_cons[blockIdx.x];
  fr_t ab[T], x[T];
  zero_many(ab);
  row_terms_many(ab, a, w, 0, a.row_ptr[0][row] + threadIdx.x, a.row_ptr[0][row + 1], 256);
  block_sum_many(ab, part);
  zero_many(x);
  row_terms_many(x, a, w, 1, a.row_ptr[1][row] + threadIdx.x, a.row_ptr[1][row + 1], 256);
  block_sum_many(x, part);
#pragma unroll
  for (u32 i = 0; i < T; i++) fe_mul(ab[i], ab[i], x[i]);
  zero_many(x);
  row_terms_many(x, a, w, 2, a.row_ptr[2][row] + threadIdx.x, a.row_ptr[2][row + 1], 256);
  block_sum_many(x, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (u32 i = 0; i < T; i++)
      if (i < w.n && !fe_eq(ab[i], x[i])) atomicMin(a.first_bad + w.first + i, row);
  }
}

static std::vector<u32> find_long_constraints(const std::vector<u32> *row_ptr_of_3) {
  std::vector<u32> v;
  for (size_t r = 0; r + 1 < row_ptr_of_3[0].size(); r++) {
    bool is_long = false;
    for (u32 m = 0; m < 3; m++) is_long |= row_ptr_of_3[m][r + 1] - row_ptr_of_3[m][r] > LONG_ROW;
    if (is_long) v.push_back((u32)r);
  }
  return v;
}

// the arguments both k-witness entry points share (what they refuse: many_strides_ok, r1cs_dev.hpp)
static void many_args(R1csManyArgs &a, const bh_r1cs *r, size_t in_stride, size_t aux_stride) {
  for (int m = 0; m < 3; m++) { a.row_ptr[m] = r->row_ptr[m]; a.terms[m] = r->terms[m]; a.out[m] = nullptr; }
  a.coeffs = r->coeffs;
  a.in_stride = in_stride; a.aux_stride = aux_stride; a.out_stride = 0;
  a.n_inputs = (u32)r->n_inputs;
  a.n_constraints = r->n_constraints;
  a.m = 0;
  a.long_rows = r->long_rows;
  a.long_cons = r->long_cons;
  a.first_bad = nullptr;
}
constexpr size_t MANY_MAX_TILES = 65535;   // a grid's second dimension

static std::vector<uint2> find_long_rows(const std::vector<u32> *row_ptr_of_3) {
  std::vector<uint2> v;
  for (u32 m = 0; m < 3; m++)
    for (size_t r = 0; r + 1 < row_ptr_of_3[m].size(); r++)
      if (row_ptr_of_3[m][r + 1] - row_ptr_of_3[m][r] > LONG_ROW) v.push_back(make_uint2(m, (u32)r));
  return v;
}

static int launch_eval(bh_ctx *ctx, R1csEvalArgs &a, u32 n_long, hipStream_t st) {
  const u64 blocks = (3 * a.m + 255) / 256, cap = (u64)ctx->c.num_cus * 16;
  hipLaunchKernelGGL(r1cs_eval_kernel, dim3((u32)(blocks < cap ? blocks : cap)), dim3(256), 0, st, a);
  BH_HIP_CHECK(hipGetLastError());
  if (n_long) {
    hipLaunchKernelGGL(r1cs_long_rows_kernel, dim3(n_long), dim3(256), 0, st, a);
    BH_HIP_CHECK(hipGetLastError());
  }
  return BH_OK;
}

template <class T>
int upload_vec(bh_ctx *ctx, T **dst, const T *src, size_t n) { return r1cs_upload_vec(ctx, dst, src, n); }

}  // namespace

namespace bh {
int r1cs_ensure_transposed(bh_ctx *ctx, bh_r1cs *r) {
  const size_t n_vars = r->n_inputs + r->n_aux;
  std::lock_guard<std::mutex> g(r->t_mu);
  if (!r->t_ready) {
    std::vector<u32> t_rp[3];
    for (int m = 0; m < 3; m++) {
      const size_t nnz = r->h_var[m].size();
      std::vector<u32> &rp = t_rp[m];
      rp.assign(n_vars + 1, 0);
      for (size_t t = 0; t < nnz; t++) rp[r->h_var[m][t] + 1]++;
      for (size_t v = 0; v < n_vars; v++) rp[v + 1] += rp[v];
      std::vector<uint2> terms(nnz);
      std::vector<u32> cursor(rp.begin(), rp.end() - 1);
      for (size_t row = 0; row < r->n_constraints; row++)
        for (u32 t = r->h_row_ptr[m][row]; t < r->h_row_ptr[m][row + 1]; t++)
          terms[cursor[r->h_var[m][t]]++] = make_uint2((u32)row, r->h_coeff[m][t]);
      int rc = upload_vec(ctx, &r->t_row_ptr[m], rp.data(), rp.size());
      if (rc == BH_OK) rc = upload_vec(ctx, &r->t_terms[m], terms.data(), nnz);
      if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
      if (rc != BH_OK) return rc;
      r->h_t_terms[m].swap(terms);   // read once more by the plan of the group-valued product (r1cs_points.hip)
    }
    const std::vector<uint2> lr = find_long_rows(t_rp);
    r->t_n_long = (u32)lr.size();
    int rc = upload_vec(ctx, &r->t_long_rows, lr.data(), lr.size());
    if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
    if (rc != BH_OK) return rc;
    r->t_ready = true;
  }
  return BH_OK;
}
}  // namespace bh

extern "C" {

int bh_r1cs_create(bh_ctx *ctx, size_t n_inputs, size_t n_aux, size_t n_constraints, const bh_csr abc[3],
                   const void *coeffs, size_t n_coeffs, bh_r1cs **out) {
  if (!ctx || !out || !abc || !coeffs || n_coeffs == 0 || n_inputs + n_aux >= (size_t(1) << 32) ||
      n_constraints >= (size_t(1) << 32))
    return BH_ERR_INVALID_ARG;
  fr_t one;
  fe_one(one);
  if (memcmp(coeffs, &one, 32) != 0) return BH_ERR_INVALID_ARG;   // slot 0 is the constant 1
  for (int m = 0; m < 3; m++) {
    if (!abc[m].row_ptr || abc[m].row_ptr[0] != 0) return BH_ERR_INVALID_ARG;
    const u32 nnz = abc[m].row_ptr[n_constraints];
    if (nnz && (!abc[m].var || !abc[m].coeff)) return BH_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_constraints; i++)
      if (abc[m].row_ptr[i] > abc[m].row_ptr[i + 1]) return BH_ERR_INVALID_ARG;
    for (u32 t = 0; t < nnz; t++)
      if (abc[m].var[t] >= n_inputs + n_aux || abc[m].coeff[t] >= n_coeffs) return BH_ERR_INVALID_ARG;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  bh_r1cs *r = new bh_r1cs;
  r->ctx = ctx;
  r->n_inputs = n_inputs; r->n_aux = n_aux; r->n_constraints = n_constraints; r->n_coeffs = n_coeffs;
  // densities: prover.rs:119-141 (A: aux only, inputs are always fully dense; B: inputs and aux; C: none),
  // zero coefficients do not count (prover.rs:31)
  const fr_t *cf = (const fr_t *)coeffs;
  std::vector<uint8_t> coeff_is_zero(n_coeffs);
  for (size_t i = 0; i < n_coeffs; i++) {
    fr_t c;
    memcpy(&c, cf + i, 32);
    coeff_is_zero[i] = fe_is_zero(c);
  }
  r->dens_host[0].assign((n_aux + 63) / 64 + 1, 0);
  r->dens_host[1].assign((n_inputs + 63) / 64 + 1, 0);
  r->dens_host[2].assign((n_aux + 63) / 64 + 1, 0);
  auto mark = [&](int which, size_t idx) { r->dens_host[which][idx >> 6] |= u64(1) << (idx & 63); };
  for (int m = 0; m < 2; m++) {
    const u32 nnz = abc[m].row_ptr[n_constraints];
    for (u32 t = 0; t < nnz; t++) {
      if (coeff_is_zero[abc[m].coeff[t]]) continue;
      const u32 v = abc[m].var[t];
      if (v >= n_inputs) mark(m == 0 ? 0 : 2, v - n_inputs);
      else if (m == 1) mark(1, v);
    }
  }
  int rc = BH_OK;
  for (int d = 0; d < 3 && rc == BH_OK; d++) {
    for (u64 w : r->dens_host[d]) r->dens_total[d] += (size_t)__builtin_popcountll(w);
    rc = upload_vec(ctx, &r->dens[d], r->dens_host[d].data(), r->dens_host[d].size());
  }
  for (int m = 0; m < 3 && rc == BH_OK; m++) {
    const u32 nnz = abc[m].row_ptr[n_constraints];
    std::vector<uint2> terms(nnz);
    for (u32 t = 0; t < nnz; t++) terms[t] = make_uint2(abc[m].var[t], abc[m].coeff[t]);
    r->h_row_ptr[m].assign(abc[m].row_ptr, abc[m].row_ptr + n_constraints + 1);
    r->h_var[m].assign(abc[m].var, abc[m].var + nnz);
    r->h_coeff[m].assign(abc[m].coeff, abc[m].coeff + nnz);
    rc = upload_vec(ctx, &r->row_ptr[m], abc[m].row_ptr, n_constraints + 1);
    if (rc == BH_OK) rc = upload_vec(ctx, &r->terms[m], terms.data(), (size_t)nnz);
    if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;   // `terms` is a local
  }
  if (rc == BH_OK) {
    const std::vector<uint2> lr = find_long_rows(r->h_row_ptr);
    r->n_long = (u32)lr.size();
    rc = upload_vec(ctx, &r->long_rows, lr.data(), lr.size());
    if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;   // `lr` is a local
  }
  if (rc == BH_OK) {
    const std::vector<u32> lc = find_long_constraints(r->h_row_ptr);
    r->n_long_cons = (u32)lc.size();
    rc = upload_vec(ctx, &r->long_cons, lc.data(), lc.size());
    if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;   // `lc` is a local
  }
  if (rc == BH_OK) rc = upload_vec(ctx, &r->coeffs, cf, n_coeffs);
  if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (rc != BH_OK) { bh_r1cs_release(r); return rc; }
  *out = r;
  return BH_OK;
}

void bh_r1cs_release(bh_r1cs *r) {
  if (!r) return;
  for (int m = 0; m < 3; m++) {
    r->ctx->c.pool.release(r->row_ptr[m]);
    r->ctx->c.pool.release(r->terms[m]);
    r->ctx->c.pool.release(r->dens[m]);
    r->ctx->c.pool.release(r->t_row_ptr[m]);
    r->ctx->c.pool.release(r->t_terms[m]);
    r->ctx->c.pool.release(r->p_terms[m]);
    r->ctx->c.pool.release(r->gen_terms[m]);
  }
  r->ctx->c.pool.release(r->coeff_canon);
  r->ctx->c.pool.release(r->coeff_info);
  r->ctx->c.pool.release(r->long_rows);
  r->ctx->c.pool.release(r->t_long_rows);
  r->ctx->c.pool.release(r->long_cons);
  r->ctx->c.pool.release(r->coeffs);
  delete r;
}

int bh_r1cs_shape(const bh_r1cs *r, size_t *n_inputs, size_t *n_aux, size_t *n_constraints) {
  if (!r) return BH_ERR_INVALID_ARG;
  if (n_inputs) *n_inputs = r->n_inputs;
  if (n_aux) *n_aux = r->n_aux;
  if (n_constraints) *n_constraints = r->n_constraints;
  return BH_OK;
}

int bh_r1cs_density(const bh_r1cs *r, int which, const uint64_t **dev_words, const uint64_t **host_words,
                    size_t *total) {
  if (!r || which < 0 || which > 2) return BH_ERR_INVALID_ARG;
  if (dev_words) *dev_words = r->dens[which];
  if (host_words) *host_words = r->dens_host[which].data();
  if (total) *total = r->dens_total[which];
  return BH_OK;
}

int bh_r1cs_eval_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, const void *aux_dev, void *a_dev,
                     void *b_dev, void *c_dev, uint32_t log_m, void *stream) {
  if (!ctx || !r || log_m >= 32 || (size_t(1) << log_m) < r->n_constraints) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  R1csEvalArgs a;
  for (int m = 0; m < 3; m++) { a.row_ptr[m] = r->row_ptr[m]; a.terms[m] = r->terms[m]; }
  a.out[0] = (fr_t *)a_dev; a.out[1] = (fr_t *)b_dev; a.out[2] = (fr_t *)c_dev;
  a.coeffs = r->coeffs; a.inputs = (const fr_t *)inputs_dev; a.aux = (const fr_t *)aux_dev;
  a.n_inputs = (u32)r->n_inputs;
  a.n_constraints = r->n_constraints;
  a.m = u64(1) << log_m;
  a.long_rows = r->long_rows;
  return launch_eval(ctx, a, r->n_long, stream ? (hipStream_t)stream : ctx->c.stream);
}

int bh_r1cs_eval_many_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, size_t in_stride, const void *aux_dev,
                          size_t aux_stride, size_t k, void *a_dev, void *b_dev, void *c_dev, size_t out_stride, uint32_t log_m,
                          void *stream) {
  constexpr u32 T = R1CS_MANY_TILE;
  if (!ctx || !r || log_m >= 32 || (size_t(1) << log_m) < r->n_constraints) return BH_ERR_INVALID_ARG;
  if (!many_strides_ok(r, inputs_dev, in_stride, aux_dev, aux_stride) || out_stride % 32 || out_stride < (size_t(32) << log_m))
    return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!a_dev || !b_dev || !c_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->c.stream;
  R1csManyArgs a;
  many_args(a, r, in_stride, aux_stride);
  a.out_stride = out_stride;
  a.m = u64(1) << log_m;
  for (size_t first = 0; first < k; first += MANY_MAX_TILES * T) {
    const size_t n = std::min<size_t>(k - first, MANY_MAX_TILES * T);
    const u32 tiles = (u32)((n + T - 1) / T);
    a.k = (u32)n;
    a.inputs = (const char *)inputs_dev + first * in_stride;
    a.aux = (const char *)aux_dev + first * aux_stride;
    a.out[0] = (char *)a_dev + first * out_stride;
    a.out[1] = (char *)b_dev + first * out_stride;
    a.out[2] = (char *)c_dev + first * out_stride;
    const u64 blocks = (3 * a.m + 255) / 256, cap = std::max<u64>((u64)ctx->c.num_cus * 16 / tiles, 1);
    hipLaunchKernelGGL(r1cs_eval_many_kernel<T>, dim3((u32)std::min(blocks, cap), tiles), dim3(256), 0, st, a);
    BH_HIP_CHECK(hipGetLastError());
    if (r->n_long) {
      hipLaunchKernelGGL(r1cs_long_rows_many_kernel<T>, dim3(r->n_long, tiles), dim3(256), 0, st, a);
      BH_HIP_CHECK(hipGetLastError());
    }
  }
  return BH_OK;
}

int bh_r1cs_check_many_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, size_t in_stride, const void *aux_dev,
                           size_t aux_stride, size_t k, uint32_t *first_bad_dev, void *stream) {
  constexpr u32 T = R1CS_MANY_TILE;
  if (!ctx || !r || !many_strides_ok(r, inputs_dev, in_stride, aux_dev, aux_stride)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!first_bad_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->c.stream;
  BH_HIP_CHECK(hipMemsetAsync(first_bad_dev, 0xFF, k * sizeof(uint32_t), st));   // BH_R1CS_SATISFIED in every word
  if (!r->n_constraints) return BH_OK;
  R1csManyArgs a;
  many_args(a, r, in_stride, aux_stride);
  for (size_t first = 0; first < k; first += MANY_MAX_TILES * T) {
    const size_t n = std::min<size_t>(k - first, MANY_MAX_TILES * T);
    const u32 tiles = (u32)((n + T - 1) / T);
    a.k = (u32)n;
    a.inputs = (const char *)inputs_dev + first * in_stride;
    a.aux = (const char *)aux_dev + first * aux_stride;
    a.first_bad = first_bad_dev + first;
    const u64 blocks = (a.n_constraints + 255) / 256, cap = std::max<u64>((u64)ctx->c.num_cus * 16 / tiles, 1);
    hipLaunchKernelGGL(r1cs_check_many_kernel<T>, dim3((u32)std::min(blocks, cap), tiles), dim3(256), 0, st, a);
    BH_HIP_CHECK(hipGetLastError());
    if (r->n_long_cons) {
      hipLaunchKernelGGL(r1cs_check_long_many_kernel<T>, dim3(r->n_long_cons, tiles), dim3(256), 0, st, a);
      BH_HIP_CHECK(hipGetLastError());
    }
  }
  return BH_OK;
}

int bh_r1cs_check_many(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_host, const void *aux_host, size_t k,
                       uint32_t *first_bad_host) {
  if (!ctx || !r) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!first_bad_host || (r->n_inputs && !inputs_host) || (r->n_aux && !aux_host)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t in_bytes = r->n_inputs * 32, aux_bytes = r->n_aux * 32;
  // groups of witnesses whose device copies stay within 1 GiB, at least one witness per group
  const size_t group = std::min(k, std::max<size_t>((size_t(1) << 30) / (in_bytes + aux_bytes + 4), 1));
  void *stream = nullptr;
  int rc = bh_stream_create(ctx, &stream);   // a stream of its own: thread-safe
  if (rc != BH_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  void *d_in = ctx->c.pool.acquire(group * in_bytes + 32), *d_aux = ctx->c.pool.acquire(group * aux_bytes + 32);
  uint32_t *d_bad = (uint32_t *)ctx->c.pool.acquire(group * sizeof(uint32_t));
  if (!d_in || !d_aux || !d_bad) rc = BH_ERR_HIP;
  auto hip_ok = [&](hipError_t e) {
    if (e != hipSuccess) {
      fprintf(stderr, "[bellman_hip] bh_r1cs_check_many: %s\n", hipGetErrorString(e));
      rc = BH_ERR_HIP;
    }
    return e == hipSuccess;
  };
  for (size_t first = 0; first < k && rc == BH_OK; first += group) {
    const size_t g = std::min(group, k - first);
    if (in_bytes && !hip_ok(hipMemcpyAsync(d_in, (const char *)inputs_host + first * in_bytes, g * in_bytes, hipMemcpyHostToDevice, st))) break;
    if (aux_bytes && !hip_ok(hipMemcpyAsync(d_aux, (const char *)aux_host + first * aux_bytes, g * aux_bytes, hipMemcpyHostToDevice, st))) break;
    rc = bh_r1cs_check_many_dev(ctx, r, d_in, in_bytes, d_aux, aux_bytes, g, d_bad, stream);
    if (rc != BH_OK) break;
    if (!hip_ok(hipMemcpyAsync(first_bad_host + first, d_bad, g * sizeof(uint32_t), hipMemcpyDeviceToHost, st))) break;
    if (!hip_ok(hipStreamSynchronize(st))) break;   // the group's buffers are written again by the next one
  }
  (void)hipStreamSynchronize(st);
  ctx->c.pool.release(d_in);
  ctx->c.pool.release(d_aux);
  ctx->c.pool.release(d_bad);
  bh_stream_destroy(ctx, stream);
  return rc;
}

// QAP polynomials at tau (generator.rs:369-387 eval_at_tau for every variable): at[v] = sum over the
// constraints j that use v in A of coeff * L_j(tau); the same sparse product as bh_r1cs_eval_dev on
// the transposed matrices, with the Lagrange coefficients in the role of the witness.
int bh_r1cs_eval_transposed_dev(bh_ctx *ctx, bh_r1cs *r, const void *lagrange_dev, void *at_dev, void *bt_dev,
                                void *ct_dev, void *stream) {
  if (!ctx || !r) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t n_vars = r->n_inputs + r->n_aux;
  {
    const int rc = r1cs_ensure_transposed(ctx, r);
    if (rc != BH_OK) return rc;
  }
  R1csEvalArgs a;
  for (int m = 0; m < 3; m++) { a.row_ptr[m] = r->t_row_ptr[m]; a.terms[m] = r->t_terms[m]; }
  a.out[0] = (fr_t *)at_dev; a.out[1] = (fr_t *)bt_dev; a.out[2] = (fr_t *)ct_dev;
  a.coeffs = r->coeffs; a.inputs = (const fr_t *)lagrange_dev; a.aux = (const fr_t *)lagrange_dev;
  a.n_inputs = 0;                       // every "variable" of the product is a constraint index
  a.n_constraints = n_vars;
  a.m = n_vars;
  if (!n_vars) return BH_OK;
  a.long_rows = r->t_long_rows;
  return launch_eval(ctx, a, r->t_n_long, stream ? (hipStream_t)stream : ctx->c.stream);
}

// generator.rs:400-407: e[v] = (at[v]*beta + bt[v]*alpha + ct[v]) * inv, inv = 1/gamma for the public
// inputs (ic) and 1/delta for the auxiliary variables (l)
int bh_fr_qap_ext_dev(bh_ctx *ctx, void *e_dev, const void *at_dev, const void *bt_dev, const void *ct_dev,
                      size_t n_inputs, size_t n_vars, const void *alpha, const void *beta, const void *gamma_inv,
                      const void *delta_inv, void *stream) {
  if (!ctx) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (!n_vars) return BH_OK;
  fr_t al, be, gi, di;
  memcpy(&al, alpha, 32); memcpy(&be, beta, 32); memcpy(&gi, gamma_inv, 32); memcpy(&di, delta_inv, 32);
  const u64 blocks = (n_vars + 255) / 256, cap = (u64)ctx->c.num_cus * 16;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->c.stream;
  hipLaunchKernelGGL(qap_ext_kernel, dim3((u32)(blocks < cap ? blocks : cap)), dim3(256), 0, st, (fr_t *)e_dev,
                     (const fr_t *)at_dev, (const fr_t *)bt_dev, (const fr_t *)ct_dev, (u64)n_inputs, (u64)n_vars, al, be,
                     gi, di);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // extern "C"
