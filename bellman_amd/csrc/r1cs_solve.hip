// The witness solver: k witnesses of one circuit completed IN PLACE on the device from the values the caller supplies.
// The reference computes every variable in a closure on one host thread while the circuit is synthesised
// (groth16/src/prover.rs:57-103 alloc / alloc_input); the matrices resident in HBM (r1cs.hip) already determine almost all
// of them: `alloc` followed by `enforce(a, b, c)` with the new variable alone in c gives v = (a * b - rest of c) / s_v.
// What the constraints cannot give - bit decompositions, inverses - comes from two kinds of hint.  The plan (which
// constraint or hint defines a variable, and the dependency level of every definition) is solve_plan.hpp, host only; this
// file holds the two launch forms that run it and the C ABI.
//
// One lane computes one (definition, witness) pair and walks the A, B and C rows of its constraint itself.
//   WALK    a workgroup owns a group of W witnesses and carries them through a run of consecutive levels in one launch,
//           lanes over (definitions of the level) x (its witnesses), a workgroup barrier between levels.  Workgroups hold
//           different witnesses and never depend on one another.
//   LEVEL   one grid-wide launch for one level; the next level is the next launch.
// Ordering between workgroups comes from launch boundaries only.  Inside the WALK kernel a level reads what other waves of
// the SAME workgroup stored in the level before: every wave drains its stores (s_waitcnt vmcnt(0) - the barrier instruction
// itself waits for no counter) and then joins __syncthreads(), whose workgroup-scope fence also keeps the compiler from
// carrying a witness value across it.  The waves of a workgroup share their CU's vector L1, which its own stores keep
// current, so no invalidate is needed - and none would be enough for another CU's stores, which is why no workgroup ever
// reads a witness another one writes.  The witness pointers carry neither const nor __restrict__: no load of them may be
// routed through the scalar or a read-only path.
#include <string.h>

#include <algorithm>
#include <vector>

#include "r1cs_dev.hpp"

using namespace bh;

namespace {

struct SolveArgs {
  const u32 *row_ptr[3];
  const uint2 *terms[3];
  const fr_t *coeffs;
  const uint4 *defs;
  const u32 *level_ptr;
  const fr_t *sinv;
  const uint2 *hint_terms;
  const u32 *out_var;
  const fr_t *hint_coeffs;
  char *inputs, *aux;       // witness j at inputs + j * in_stride, aux + j * aux_stride; read AND written
  u64 in_stride, aux_stride;
  u64 k;                    // witnesses of this launch
  u32 n_inputs;
  u32 level_lo, level_hi;   // WALK: the run of levels; LEVEL: level_lo alone
  u32 w;                    // WALK: witnesses per workgroup
};

__device__ __forceinline__ fr_t *var_slot(char *in, char *aux, u32 n_inputs, u32 var) {
  return var < n_inputs ? reinterpret_cast<fr_t *>(in) + var : reinterpret_cast<fr_t *>(aux) + (var - n_inputs);
}

// sum over the terms [lo, hi) of coefficient * variable, the terms of variable `skip` left out
__device__ __forceinline__ fr_t walk_terms(const uint2 *terms, const fr_t *coeffs, u32 lo, u32 hi, u32 skip, char *in, char *aux,
                                           u32 n_inputs) {
  fr_t acc;
  fe_zero(acc);
  for (u32 t = lo; t < hi; t++) {
    const uint2 term = terms[t];
    if (term.x == skip) continue;
    fr_t w = ld_fr16(var_slot(in, aux, n_inputs, term.x));
    if (term.y != 0) {   // entry 0 of both coefficient tables is 1
      const fr_t c = ld_fr16(coeffs + term.y);
      fe_mul(w, w, c);
    }
    fe_add(acc, acc, w);
  }
  return acc;
}

// out of line: ~380 products of a lane that meets an INV_OR_ZERO hint must not sit in every other lane's registers
__device__ __attribute__((noinline)) fr_t inverse_or_zero(fr_t x) {
  if (fe_is_zero(x)) return x;
  fr_t r;
  fe_inv(r, x);
  return r;
}

// one definition for one witness
__device__ __forceinline__ void solve_one(const SolveArgs &a, u32 d, char *in, char *aux) {
  const uint4 d0 = a.defs[2 * (u64)d], d1 = a.defs[2 * (u64)d + 1];
  const u32 kind = d0.x, index = d0.y, var = d0.z, mode = d0.w, da = d1.x, db = d1.y, count = d1.z;
  if (kind == SOLVE_DEF_CONSTRAINT) {
    const u32 none = 0xFFFFFFFFu;   // n_vars < 2^32: never a variable
    fr_t x = walk_terms(a.terms[0], a.coeffs, a.row_ptr[0][index], a.row_ptr[0][index + 1], none, in, aux, a.n_inputs);
    const fr_t y = walk_terms(a.terms[1], a.coeffs, a.row_ptr[1][index], a.row_ptr[1][index + 1], none, in, aux, a.n_inputs);
    fe_mul(x, x, y);
    const fr_t rest = walk_terms(a.terms[2], a.coeffs, a.row_ptr[2][index], a.row_ptr[2][index + 1], var, in, aux, a.n_inputs);
    fe_sub(x, x, rest);
    if (mode == SOLVE_S_MINUS_ONE) {
      fe_neg(x, x);
    } else if (mode == SOLVE_S_GENERAL) {
      const fr_t si = ld_fr16(a.sinv + da);
      fe_mul(x, x, si);
    }
    st_fr16(var_slot(in, aux, a.n_inputs, var), x);
    return;
  }
  fr_t x = walk_terms(a.hint_terms, a.hint_coeffs, da, db, 0xFFFFFFFFu, in, aux, a.n_inputs);
  if (kind == SOLVE_DEF_INV_OR_ZERO) {
    x = inverse_or_zero(x);
    st_fr16(var_slot(in, aux, a.n_inputs, a.out_var[var]), x);
    return;
  }
  // SOLVE_DEF_BITS: bits mode .. mode + count of the canonical integer (mode + count <= 256: the plan)
  fr_t canon, one, zero;
  fe_from_mont(canon, x);
  fe_one(one);
  fe_zero(zero);
  for (u32 j = 0; j < count; j++) {
    const u32 bit = mode + j;
    u32 limb = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++) limb = (bit >> 5) == i ? canon.l[i] : limb;   // (no dynamic index: canon stays in registers)
    st_fr16(var_slot(in, aux, a.n_inputs, a.out_var[var + j]), ((limb >> (bit & 31)) & 1) ? one : zero);
  }
}

__global__ void __launch_bounds__(SOLVE_WALK_LANES) r1cs_solve_walk_kernel(SolveArgs a) {
  const u64 first = (u64)blockIdx.x * a.w;
  const u32 nw = (u32)(a.k - first < a.w ? a.k - first : a.w);   // the grid has no workgroup beyond k
  for (u32 level = a.level_lo; level < a.level_hi; level++) {
    const u32 lo = a.level_ptr[level], width = a.level_ptr[level + 1] - lo;
    const u64 items = (u64)width * nw;
    for (u64 i = threadIdx.x; i < items; i += SOLVE_WALK_LANES) {
      const u32 d = (u32)(i / nw);
      const u64 j = first + (i - (u64)d * nw);
      solve_one(a, lo + d, a.inputs + j * a.in_stride, a.aux + j * a.aux_stride);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores have left before it reaches the barrier
    __syncthreads();
  }
}

__global__ void __launch_bounds__(SOLVE_WALK_LANES) r1cs_solve_level_kernel(SolveArgs a) {
  const u32 lo = a.level_ptr[a.level_lo], width = a.level_ptr[a.level_lo + 1] - lo;
  const u64 items = (u64)width * a.k;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x) {
    const u64 j = i / width;
    const u32 d = (u32)(i - j * width);
    solve_one(a, lo + d, a.inputs + j * a.in_stride, a.aux + j * a.aux_stride);
  }
}

constexpr u64 WALK_MAX_GROUPS = (u64)1 << 30;   // workgroups of one launch

}  // namespace

extern "C" {

int bh_r1cs_solver_create(bh_ctx *ctx, const bh_r1cs *r, const bh_solver_desc *desc, uint32_t *first_unsolved,
                          bh_r1cs_solver **out) {
  if (first_unsolved) *first_unsolved = SOLVE_NO_VAR;
  if (!ctx || !r || !desc || !out || r->ctx != ctx) return BH_ERR_INVALID_ARG;
  if ((desc->n_supplied && !desc->supplied) || (desc->n_hints && (!desc->hints || !desc->out_var || !desc->hint_coeffs)))
    return BH_ERR_INVALID_ARG;
  static_assert(sizeof(bh_witness_hint) == sizeof(SolveHint) && sizeof(SolveDef) == 2 * sizeof(uint4), "record layouts");
  fr_t one;
  fe_one(one);
  if (desc->n_hints && (!desc->n_hint_coeffs || memcmp(desc->hint_coeffs, &one, 32) != 0)) return BH_ERR_INVALID_ARG;
  SolveDesc d;
  d.supplied = desc->supplied; d.n_supplied = desc->n_supplied;
  d.hints = reinterpret_cast<const SolveHint *>(desc->hints); d.n_hints = desc->n_hints;
  d.lc_var = desc->lc_var; d.lc_coeff = desc->lc_coeff; d.out_var = desc->out_var;
  d.n_lc = d.n_out = 0;
  for (size_t h = 0; h < desc->n_hints; h++) {
    d.n_lc = std::max<size_t>(d.n_lc, desc->hints[h].lc_end);
    d.n_out = std::max<size_t>(d.n_out, desc->hints[h].out_end);
  }
  if (d.n_lc && (!desc->lc_var || !desc->lc_coeff)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  // the circuit's coefficient table lives on the device alone
  std::vector<fr_t> coeffs(r->n_coeffs);
  BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  BH_HIP_CHECK(hipMemcpy(coeffs.data(), r->coeffs, r->n_coeffs * sizeof(fr_t), hipMemcpyDeviceToHost));
  std::vector<fr_t> hint_coeffs(desc->n_hints ? desc->n_hint_coeffs : 0);
  if (!hint_coeffs.empty()) memcpy(hint_coeffs.data(), desc->hint_coeffs, hint_coeffs.size() * sizeof(fr_t));
  SolveCsr abc[3];
  for (int m = 0; m < 3; m++) abc[m] = SolveCsr{r->h_row_ptr[m].data(), r->h_var[m].data(), r->h_coeff[m].data()};
  const SolvePlan<fr_t> p = solve_plan(SolveFr(), r->n_inputs + r->n_aux, r->n_constraints, abc, coeffs.data(), coeffs.size(), d,
                                       hint_coeffs.data(), hint_coeffs.size());
  if (p.status != SOLVE_OK) {
    if (first_unsolved) *first_unsolved = p.first_unsolved;
    return BH_ERR_INVALID_ARG;
  }
  bh_r1cs_solver *s = new bh_r1cs_solver;
  s->ctx = ctx;
  s->r = r;
  s->h_level_ptr = p.level_ptr;
  s->counts[0] = p.n_supplied; s->counts[1] = p.n_defined; s->counts[2] = p.n_hinted;
  s->counts[3] = p.level_ptr.size() - 1; s->counts[4] = p.widest;
  std::vector<uint2> hint_terms(d.n_lc);
  for (size_t t = 0; t < d.n_lc; t++) hint_terms[t] = make_uint2(desc->lc_var[t], desc->lc_coeff[t]);
  int rc = r1cs_upload_vec(ctx, &s->defs, reinterpret_cast<const uint4 *>(p.defs.data()), 2 * p.defs.size());
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &s->level_ptr, p.level_ptr.data(), p.level_ptr.size());
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &s->sinv, p.sinv.data(), p.sinv.size());
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &s->hint_terms, hint_terms.data(), hint_terms.size());
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &s->out_var, desc->out_var, d.n_out);
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &s->hint_coeffs, hint_coeffs.data(), hint_coeffs.size());
  if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;   // the sources are locals
  if (rc != BH_OK) { bh_r1cs_solver_release(s); return rc; }
  *out = s;
  return BH_OK;
}

void bh_r1cs_solver_release(bh_r1cs_solver *s) {
  if (!s) return;
  s->ctx->c.pool.release(s->defs);
  s->ctx->c.pool.release(s->level_ptr);
  s->ctx->c.pool.release(s->sinv);
  s->ctx->c.pool.release(s->hint_terms);
  s->ctx->c.pool.release(s->out_var);
  s->ctx->c.pool.release(s->hint_coeffs);
  delete s;
}

int bh_r1cs_solver_info(const bh_r1cs_solver *s, size_t counts[5]) {
  if (!s || !counts) return BH_ERR_INVALID_ARG;
  for (int i = 0; i < 5; i++) counts[i] = s->counts[i];
  return BH_OK;
}

int bh_r1cs_solve_many_dev(bh_ctx *ctx, const bh_r1cs_solver *s, void *inputs_dev, size_t in_stride, void *aux_dev,
                           size_t aux_stride, size_t k, void *stream) {
  if (!ctx || !s || s->ctx != ctx || !many_strides_ok(s->r, inputs_dev, in_stride, aux_dev, aux_stride)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->c.stream;
  const bh_r1cs *r = s->r;
  SolveArgs a;
  for (int m = 0; m < 3; m++) { a.row_ptr[m] = r->row_ptr[m]; a.terms[m] = r->terms[m]; }
  a.coeffs = r->coeffs;
  a.defs = s->defs; a.level_ptr = s->level_ptr; a.sinv = s->sinv;
  a.hint_terms = s->hint_terms; a.out_var = s->out_var; a.hint_coeffs = s->hint_coeffs;
  a.in_stride = in_stride; a.aux_stride = aux_stride;
  a.n_inputs = (u32)r->n_inputs;
  const std::vector<u32> &lp = s->h_level_ptr;
  const u32 levels = (u32)(lp.size() - 1);
  auto is_level_form = [&](u32 l) {
    if (s->force_form != SOLVE_FORM_AUTO) return s->force_form == SOLVE_FORM_LEVEL;
    return (u64)(lp[l + 1] - lp[l]) * k >= s->level_min_items;
  };
  for (u32 l = 0; l < levels;) {
    if (is_level_form(l)) {
      a.inputs = (char *)inputs_dev; a.aux = (char *)aux_dev;
      a.k = k; a.level_lo = l; a.level_hi = l + 1; a.w = 0;
      const u64 items = (u64)(lp[l + 1] - lp[l]) * k;
      const u64 blocks = (items + SOLVE_WALK_LANES - 1) / SOLVE_WALK_LANES, cap = (u64)ctx->c.num_cus * 16;
      hipLaunchKernelGGL(r1cs_solve_level_kernel, dim3((u32)std::min(blocks, cap)), dim3(SOLVE_WALK_LANES), 0, st, a);
      BH_HIP_CHECK(hipGetLastError());
      l++;
      continue;
    }
    u32 e = l + 1;
    while (e < levels && !is_level_form(e)) e++;
    u32 w = s->force_w;
    if (!w) {   // a wavefront's worth of pairs per level at the run's mean width (r1cs_dev.hpp has the sweep)
      const u64 mean = std::max<u64>((lp[e] - lp[l]) / (e - l), 1);
      w = (u32)std::min<u64>(std::max<u64>(SOLVE_WALK_ITEMS / mean, 1), SOLVE_WALK_MAX_W);
    }
    a.level_lo = l; a.level_hi = e; a.w = w;
    for (size_t first = 0; first < k; first += WALK_MAX_GROUPS * w) {
      const size_t n = std::min<size_t>(k - first, WALK_MAX_GROUPS * w);
      a.inputs = (char *)inputs_dev + first * in_stride;
      a.aux = (char *)aux_dev + first * aux_stride;
      a.k = n;
      hipLaunchKernelGGL(r1cs_solve_walk_kernel, dim3((u32)((n + w - 1) / w)), dim3(SOLVE_WALK_LANES), 0, st, a);
      BH_HIP_CHECK(hipGetLastError());
    }
    l = e;
  }
  return BH_OK;
}

int bh_r1cs_solve_many(bh_ctx *ctx, const bh_r1cs_solver *s, void *inputs_host, void *aux_host, size_t k) {
  if (!ctx || !s || s->ctx != ctx) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  const bh_r1cs *r = s->r;
  if ((r->n_inputs && !inputs_host) || (r->n_aux && !aux_host)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t in_bytes = r->n_inputs * 32, aux_bytes = r->n_aux * 32;
  // groups of witnesses whose device copies stay within 1 GiB, at least one witness per group
  const size_t group = std::min(k, std::max<size_t>((size_t(1) << 30) / (in_bytes + aux_bytes), 1));
  void *stream = nullptr;
  int rc = bh_stream_create(ctx, &stream);   // a stream of its own: thread-safe
  if (rc != BH_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  void *d_in = ctx->c.pool.acquire(group * in_bytes + 32), *d_aux = ctx->c.pool.acquire(group * aux_bytes + 32);
  if (!d_in || !d_aux) rc = BH_ERR_HIP;
  auto hip_ok = [&](hipError_t e) {
    if (e != hipSuccess) {
      fprintf(stderr, "[bellman_hip] bh_r1cs_solve_many: %s\n", hipGetErrorString(e));
      rc = BH_ERR_HIP;
    }
    return e == hipSuccess;
  };
  for (size_t first = 0; first < k && rc == BH_OK; first += group) {
    const size_t g = std::min(group, k - first);
    char *h_in = (char *)inputs_host + first * in_bytes, *h_aux = (char *)aux_host + first * aux_bytes;
    if (in_bytes && !hip_ok(hipMemcpyAsync(d_in, h_in, g * in_bytes, hipMemcpyHostToDevice, st))) break;
    if (aux_bytes && !hip_ok(hipMemcpyAsync(d_aux, h_aux, g * aux_bytes, hipMemcpyHostToDevice, st))) break;
    rc = bh_r1cs_solve_many_dev(ctx, s, d_in, in_bytes, d_aux, aux_bytes, g, stream);
    if (rc != BH_OK) break;
    if (in_bytes && !hip_ok(hipMemcpyAsync(h_in, d_in, g * in_bytes, hipMemcpyDeviceToHost, st))) break;
    if (aux_bytes && !hip_ok(hipMemcpyAsync(h_aux, d_aux, g * aux_bytes, hipMemcpyDeviceToHost, st))) break;
    if (!hip_ok(hipStreamSynchronize(st))) break;   // the group's buffers are written again by the next one
  }
  (void)hipStreamSynchronize(st);
  ctx->c.pool.release(d_in);
  ctx->c.pool.release(d_aux);
  bh_stream_destroy(ctx, stream);
  return rc;
}

}  // extern "C"
