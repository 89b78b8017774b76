// The device-resident R1CS handle (bh_r1cs), shared by r1cs.hip (products with Fr vectors), r1cs_points.hip
// (products with vectors of group elements), r1cs_solve.hip (witnesses completed from their supplied values) and
// word_witness.hip (witnesses computed from a gadget circuit's word program).
#pragma once
#include <mutex>
#include <vector>

#include "common.hpp"
#include "solve_plan.hpp"
#include "word_program.hpp"

// A row with more terms than this is summed by a whole workgroup instead of one lane: the constant
// ONE typically appears in every constraint, so its row of a transposed matrix has ~n terms.
namespace bh {
constexpr u32 LONG_ROW = 1024;
// Witnesses per lane of the k-witness kernels (r1cs.hip: r1cs_eval_many_kernel, r1cs_check_many_kernel): a lane reads a term
// record and its coefficient once and applies them to this many witnesses.  The largest of 2, 4, 8 at which clang reports no
// scratch and at most 128 VGPRs for every one of those kernels (tools/kernel_resources.py r1cs.hip; the line is in DESIGN.md
// 5.4.1): the kernels are bound by the latency of the witness gathers and want waves in flight.
constexpr u32 R1CS_MANY_TILE = 2;

// The solver's launch forms (r1cs_solve.hip).  A level of `width` definitions over k witnesses is one grid-wide launch of its
// own (LEVEL) when width * k reaches SOLVE_LEVEL_MIN_ITEMS; the levels between two such levels are ONE launch (WALK) in which a
// workgroup carries W = SOLVE_WALK_ITEMS / (mean width of the run) witnesses, at least 1 and at most SOLVE_WALK_MAX_W,
// through all of them.  tools/bench_r1cs_solve.py --sweep -> profiles/r1cs_solve_bench_w256.json, the run that chose W:
//   W      one wavefront's worth of (definition, witness) pairs per level.  Boolean circuit 2^16 x 256 (mean width 19): W = 1 / 4 /
//          16 / 64 -> 81.1 / 80.0 / 96.7 / 128.5 ms; chain 2^14 x 256 (width 1): 71.1 / 71.9 / 70.8 / 67.9 ms.
//   switch NOT settled by the sweep: no level of the measured circuits reaches 2^14 items at k = 256 (widest level 29), and one
//          launch per level throughout loses 1.5 - 2.3 x.  The value stands by reasoning: a launch boundary costs about as much
//          as four barrier-separated passes of a workgroup, so a level earns a launch where every CU would need that many.
constexpr u32 SOLVE_WALK_LANES = 256;          // lanes of a workgroup of both kernels
constexpr u32 SOLVE_WALK_ITEMS = 64;
constexpr u32 SOLVE_WALK_MAX_W = 64;
constexpr u64 SOLVE_LEVEL_MIN_ITEMS = (u64)1 << 18;   // 256 CUs x 256 lanes x 4
enum : u32 { SOLVE_FORM_AUTO = 0, SOLVE_FORM_WALK = 1, SOLVE_FORM_LEVEL = 2 };

// The word-program witness generator (word_witness.hip).  The run kernel gives every witness one lane, so a workgroup is one
// wavefront: k witnesses spread over k / 64 CUs.  The expansion writes 32 bytes per lane, 256 consecutive variables of one
// witness per workgroup.  Witnesses go through in chunks whose scratch word file (8 bytes x words x witnesses) stays within
// WORD_SCRATCH_MAX_BYTES: 256 MiB hold 21 000 witnesses of a one-block SHA-256 (1 555 words) - beyond that a chunk's two
// launches are long enough (tens of ms at HBM store speed) that one more pair costs nothing measurable.  Not swept.
constexpr u32 WORD_RUN_LANES = 64;
constexpr u32 WORD_EXPAND_LANES = 256;
constexpr u64 WORD_SCRATCH_MAX_BYTES = (u64)256 << 20;

// the 16-byte halves of an Fr record (the witness vectors are 32-byte aligned: bh_dev_alloc, strides multiples of 32)
__device__ __forceinline__ fr_t ld_fr16(const fr_t *p) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  uint4 lo = q[0], hi = q[1];
  fr_t r;
  r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
  r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
  return r;
}
__device__ __forceinline__ void st_fr16(fr_t *p, const fr_t &r) {
  uint4 *q = reinterpret_cast<uint4 *>(p);
  q[0] = make_uint4(r.l[0], r.l[1], r.l[2], r.l[3]);
  q[1] = make_uint4(r.l[4], r.l[5], r.l[6], r.l[7]);
}

// the field of solve_plan.hpp: Montgomery Fr of ff.cuh on the host
struct SolveFr {
  typedef fr_t Elem;
  static fr_t zero() { fr_t z; fe_zero(z); return z; }
  static bool is_zero(const fr_t &a) { return fe_is_zero(a); }
  static fr_t add(const fr_t &a, const fr_t &b) { fr_t r; fe_add(r, a, b); return r; }
  static bool is_one(const fr_t &a) { fr_t o; fe_one(o); return fe_eq(a, o); }
  static bool is_minus_one(const fr_t &a) { fr_t o; fe_one(o); fe_neg(o, o); return fe_eq(a, o); }
  static fr_t inv(const fr_t &a) { fr_t r; fe_inv(r, a); return r; }
};
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

// A witness solver of one circuit (bh_r1cs_solver_create): the plan of solve_plan.hpp on the device.  The three tuning
// words are written by the test library alone (bh_test_r1cs_solver_tune), between calls.
struct bh_r1cs_solver {
  bh_ctx *ctx = nullptr;
  const bh_r1cs *r = nullptr;
  uint4 *defs = nullptr;                 // bh::SolveDef records, sorted by level
  bh::u32 *level_ptr = nullptr;
  bh::fr_t *sinv = nullptr;
  uint2 *hint_terms = nullptr;           // (variable, entry of hint_coeffs)
  bh::u32 *out_var = nullptr;
  bh::fr_t *hint_coeffs = nullptr;
  std::vector<bh::u32> h_level_ptr;
  size_t counts[5] = {0, 0, 0, 0, 0};    // supplied, defined, hinted, levels, widest level
  bh::u32 force_form = bh::SOLVE_FORM_AUTO, force_w = 0;
  bh::u64 level_min_items = bh::SOLVE_LEVEL_MIN_ITEMS;
};

// A word program on the device (bh_word_witness_create).  The scratch word file belongs to the handle and is reused by its
// calls: `mu` serialises their enqueueing, `done` orders a call behind the previous one on whatever stream that ran.
// force_chunk is written by the test library alone (bh_test_word_witness_chunk), between calls.
struct bh_word_witness {
  bh_ctx *ctx = nullptr;
  size_t n_inputs = 0, n_aux = 0, n_ext = 0, n_instrs = 0, n_words = 0;
  uint4 *instrs = nullptr;               // bh::WordInstr
  bh::u32 *pool = nullptr;
  uint2 *bits = nullptr;                 // bh::WordBit
  uint2 *recs = nullptr;                 // bh::WordRec, per variable
  std::mutex mu;
  bh::u64 *scratch = nullptr;
  size_t scratch_bytes = 0;
  hipEvent_t done = nullptr;
  bool used = false;
  size_t force_chunk = 0;
};

namespace bh {
// the field of word_program.hpp: Montgomery Fr of ff.cuh on the host
struct WordFr {
  typedef fr_t Elem;
  static fr_t zero() { fr_t z; fe_zero(z); return z; }
  static fr_t one() { fr_t o; fe_one(o); return o; }
  static fr_t from_canonical(const uint64_t limbs[4]) {
    fr_t c, r;
    for (int i = 0; i < 4; i++) { c.l[2 * i] = (u32)limbs[i]; c.l[2 * i + 1] = (u32)(limbs[i] >> 32); }
    fe_to_mont(r, c);
    return r;
  }
};
// what the k-witness entry points refuse in their witness buffers
inline bool many_strides_ok(const bh_r1cs *r, const void *inputs_dev, size_t in_stride, const void *aux_dev, size_t aux_stride) {
  return in_stride % 32 == 0 && aux_stride % 32 == 0 && in_stride >= r->n_inputs * 32 && aux_stride >= r->n_aux * 32 &&
         (inputs_dev || !r->n_inputs) && (aux_dev || !r->n_aux);
}
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
