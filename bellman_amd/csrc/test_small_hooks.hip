// libbellman_hip_test.so: the two kernels of msm_accumulate.cuh outside the staged pipeline, each on its own -
// msm_small_fill_kernel, the one-launch path that replaces stages 1 - 4 of a small multiexp over a window table, through the
// plan and the launch function msm_enqueue uses (make_table_plan, small_fill_plan of msm_stage_plans.hpp, launch_small_fill of
// msm_ec.cuh), in its four instantiations, over scalars, a density and a TABLE of the caller's choice; and
// msm_err_resolve_kernel through what msm_finish uses (err_resolve_lo_ref, launch_err_resolve).  Everything the kernels wrote
// comes back raw (bh_test_small_fill_* and bh_test_err_resolve_* of include/bellman_hip_test.h; tests/test_gpu_small_fill.py,
// tests/test_small_fill_model_cpu.py, tests/models/small_fill_model.py).  Every argument is validated on the host before
// anything is launched: a shape the shipped plan does not fuse, or a base cursor that could leave the table, is refused.
// Every device buffer has its exact production element count - no rounding to 256 bytes - and a guard behind it.
#include <string.h>

#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_ec.cuh"

namespace bh {
namespace smallfill {

constexpr size_t GUARD = 4096;                       // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;             // what the buffers production takes unzeroed from the pool hold here
constexpr u64 MAX_ROW_RECORDS = (u64)1 << 16, MAX_RESOLVE = (u64)1 << 20;
constexpr int PLAN_NUM_CUS = 256;                    // make_table_plan sizes the chunks of the staged path by it: nothing here reads them
enum { FORM_FP, FORM_FP2K3, FORM_FP2PAIR, FORM_FP2, FORMS };
enum { PL_FUSED, PL_WORKGROUPS, PL_THREADS, PL_LDS, PL_BPB, PL_TOP_BITS, PL_SLIVER, PL_WD, PL_ENTRIES, PL_NB, PL_MAX_SCALARS, PL_MAX_ENTRIES,
       PL_MAX_PER_BUCKET, PL_LIST_CAP, PL_LANES_PER_BUCKET, PL_XYZZ, PL_AFFINE, PL_GUARD, PL_SENTINEL, PL_ERR_BYTES, PL_WORDS };
enum { G_PTS, G_WORD_PREFIX, G_ERR, G_SCALARS, G_DENSITY, G_TABLE, G_WORDS };
enum { R_SCALARS, R_DENSITY, R_WORD_PREFIX, R_BASES, R_ERR, R_WORDS };

static u32 form_workers(int form) {
  switch (form) {
    case FORM_FP: return small_fill_workers<FpOps>();
    case FORM_FP2K3: return small_fill_workers<Fp2K3Ops>();
    case FORM_FP2PAIR: return small_fill_workers<Fp2PairOps>();
    default: return small_fill_workers<Fp2Ops>();
  }
}
// the conditions of msm_enqueue and msm_pick_sources on a table plan: 32-bit pair positions, 31-bit row indices
static bool plan_args_ok(int form, u64 nd, u32 c, u64 row_records) {
  if (form < 0 || form >= FORMS || !nd || c < 2 || c > 24 || !row_records) return false;
  const u64 Wd = (256 + c - 1) / c;
  return nd < ((u64)1 << 32) && Wd * nd < ((u64)1 << 32) && Wd * row_records < ((u64)1 << 31);
}
// the shipped plans of a table of ceil(256 / c) rows of row_records records at the dense stride (MsmSources::small_path)
static SmallFillPlan stage_plans(int form, u64 nd, u32 c, u64 row_records, u32 flags, MsmPlan &p) {
  WindowTable t;
  t.c = c; t.W = (256 + c - 1) / c; t.stride = row_records;
  p = make_table_plan(nd, t, 0, form != FORM_FP, PLAN_NUM_CUS);
  return small_fill_plan(p, true, false, flags, form_workers(form));
}

// a Montgomery scalar has to be a field element (< q): fe_from_mont is defined for those alone
static const u32 FR_MODULUS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
static bool below_modulus(const u32 *s) {
  for (int i = 7; i >= 0; i--)
    if (s[i] != FR_MODULUS[i]) return s[i] < FR_MODULUS[i];
  return false;
}
static bool scalars_ok(const void *scalars, int fmt, size_t nd) {
  if (fmt != BH_SCALARS_CANONICAL && fmt != BH_SCALARS_MONT) return false;
  if (fmt == BH_SCALARS_MONT)
    for (size_t i = 0; i < nd; i++)
      if (!below_modulus((const u32 *)scalars + 8 * i)) return false;
  return true;
}

struct DevBuf {   // `bytes` of payload + GUARD, freed on scope exit
  char *p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t n, int fill, hipStream_t st) {
    bytes = n;
    BH_HIP_CHECK(hipMalloc((void **)&p, n + GUARD));
    if (n) BH_HIP_CHECK(hipMemsetAsync(p, fill, n, st));
    BH_HIP_CHECK(hipMemsetAsync(p + n, SENTINEL, GUARD, st));
    return BH_OK;
  }
  int upload(const void *host, hipStream_t st) {
    if (bytes) BH_HIP_CHECK(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, st));
    return BH_OK;
  }
  // the payload into `host` (optional), the guard into `guard`
  int fetch(void *host, std::vector<unsigned char> &guard, hipStream_t st) const {
    guard.resize(GUARD);
    if (host && bytes) BH_HIP_CHECK(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, st));
    BH_HIP_CHECK(hipMemcpyAsync(guard.data(), p + bytes, GUARD, hipMemcpyDeviceToHost, st));
    return BH_OK;
  }
};
static u32 guard_intact(const std::vector<unsigned char> &g) {
  for (unsigned char b : g)
    if (b != SENTINEL) return 0;
  return 1;
}

template <class F>
static int run_small_fill(hipStream_t st, const MsmPlan &p, const SmallFillPlan &sp, const void *scalars, int fmt, const u64 *density,
                          u32 *word_prefix, u64 skip, u64 n_bases, const void *table, void *pts, ErrFlags *err) {
  typedef typename F::Mem M;
  return launch_small_fill<F>(st, p, sp, scalars, fmt, density, word_prefix, skip, n_bases, (const Affine<M> *)table, (XYZZ<M> *)pts, err);
}
}  // namespace smallfill
}  // namespace bh

using namespace bh;
using namespace bh::smallfill;
extern "C" {
int bh_test_small_fill_plan(int form, size_t nd, unsigned c, size_t row_records, uint32_t flags, uint64_t plan_out20[20]) {
  static_assert(PL_WORDS == 20, "include/bellman_hip_test.h documents 20 words");
  if (!plan_out20 || !plan_args_ok(form, nd, c, row_records)) return BH_ERR_INVALID_ARG;
  MsmPlan p;
  const SmallFillPlan sp = stage_plans(form, nd, c, row_records, flags, p);
  u64 *out = plan_out20;
  out[PL_FUSED] = sp.fused ? 1 : 0; out[PL_WORKGROUPS] = sp.workgroups; out[PL_THREADS] = sp.threads; out[PL_LDS] = sp.lds_bytes;
  out[PL_BPB] = sp.buckets_per_workgroup; out[PL_TOP_BITS] = sp.top_bits; out[PL_SLIVER] = sp.sliver_load;
  out[PL_WD] = p.Wd; out[PL_ENTRIES] = p.n; out[PL_NB] = p.nb;
  out[PL_MAX_SCALARS] = SMALL_MAX_SCALARS; out[PL_MAX_ENTRIES] = SMALL_MAX_ENTRIES; out[PL_MAX_PER_BUCKET] = SMALL_MAX_PER_BUCKET;
  out[PL_LIST_CAP] = SMALL_LIST_CAP; out[PL_LANES_PER_BUCKET] = SMALL_LANES_PER_BUCKET;
  out[PL_XYZZ] = form == FORM_FP ? sizeof(XYZZ<FpOps>) : sizeof(XYZZ<Fp2Ops>);
  out[PL_AFFINE] = form == FORM_FP ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  out[PL_GUARD] = GUARD; out[PL_SENTINEL] = SENTINEL; out[PL_ERR_BYTES] = sizeof(ErrFlags);
  return BH_OK;
}
int bh_test_small_fill_dev(bh_ctx *ctx, int form, unsigned c, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                           size_t skip, size_t n_bases, const void *table, size_t row_records, void *pts_out,
                           uint32_t *word_prefix_out, void *err_out, uint32_t guards_out6[6]) {
  static_assert(G_WORDS == 6, "include/bellman_hip_test.h documents 6 guard flags");
  if (!ctx || !scalars || !table || !pts_out || !err_out || !guards_out6) return BH_ERR_INVALID_ARG;
  if (!plan_args_ok(form, nd, c, row_records) || row_records > MAX_ROW_RECORDS) return BH_ERR_INVALID_ARG;
  if ((density_words != nullptr) != (word_prefix_out != nullptr)) return BH_ERR_INVALID_ARG;
  // the base cursor of a live scalar is below n_bases: inside a row of the table
  if (n_bases > row_records || skip >= ((size_t)1 << 31)) return BH_ERR_INVALID_ARG;
  MsmPlan p;
  const SmallFillPlan sp = stage_plans(form, nd, c, row_records, 0, p);
  if (!sp.fused || !sp.workgroups || p.c != c || p.nd != nd) return BH_ERR_INVALID_ARG;
  if (!scalars_ok(scalars, fmt, nd)) return BH_ERR_INVALID_ARG;
  const size_t rec = form == FORM_FP ? sizeof(XYZZ<FpOps>) : sizeof(XYZZ<Fp2Ops>);
  const size_t arec = form == FORM_FP ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  const size_t nwords = (nd + 63) / 64;

  Context &cx = ctx->c;
  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_scalars, d_density, d_table, d_err, d_pts, d_prefix;
  int rc;
  if ((rc = d_scalars.alloc(nd * 32, 0, st)) || (rc = d_scalars.upload(scalars, st)) ||
      (rc = d_table.alloc((size_t)p.Wd * row_records * arec, 0, st)) || (rc = d_table.upload(table, st)) ||
      // zeroed, as in production: the status words and the buckets (all-zero XYZZ == identity)
      (rc = d_err.alloc(sizeof(ErrFlags), 0, st)) || (rc = d_pts.alloc((size_t)p.nb * rec, 0, st)))
    return rc;
  if (density_words &&
      ((rc = d_density.alloc(nwords * 8, 0, st)) || (rc = d_density.upload(density_words, st)) ||
       // from the pool, not zeroed
       (rc = d_prefix.alloc((nwords + 1) * 4, SENTINEL, st))))
    return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copies above may still be staged)
  const u64 *dens = density_words ? (const u64 *)d_density.p : nullptr;
  u32 *prefix = density_words ? (u32 *)d_prefix.p : nullptr;
  ErrFlags *err = (ErrFlags *)d_err.p;
#define BH_SMALL(F) run_small_fill<F>(st, p, sp, d_scalars.p, fmt, dens, prefix, skip, n_bases, d_table.p, d_pts.p, err)
  rc = form == FORM_FP ? BH_SMALL(FpOps) : form == FORM_FP2K3 ? BH_SMALL(Fp2K3Ops) : form == FORM_FP2PAIR ? BH_SMALL(Fp2PairOps) : BH_SMALL(Fp2Ops);
#undef BH_SMALL
  if (rc) return rc;
  std::vector<unsigned char> g[G_WORDS];
  if ((rc = d_pts.fetch(pts_out, g[G_PTS], st)) || (rc = d_err.fetch(err_out, g[G_ERR], st)) ||
      (rc = d_scalars.fetch(nullptr, g[G_SCALARS], st)) || (rc = d_table.fetch(nullptr, g[G_TABLE], st)))
    return rc;
  if (density_words && ((rc = d_prefix.fetch(word_prefix_out, g[G_WORD_PREFIX], st)) || (rc = d_density.fetch(nullptr, g[G_DENSITY], st)))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < G_WORDS; k++) guards_out6[k] = g[k].empty() ? 1u : guard_intact(g[k]);
  return BH_OK;
}
uint32_t bh_test_err_resolve_lo_ref(uint64_t nref) { return err_resolve_lo_ref(nref); }
int bh_test_err_resolve_dev(bh_ctx *ctx, int group, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                            const uint32_t *word_prefix, size_t skip, size_t n_bases, const void *bases, size_t n_records,
                            unsigned base_stride, uint64_t ref_n, void *err_inout, uint32_t guards_out5[5]) {
  static_assert(R_WORDS == 5, "include/bellman_hip_test.h documents 5 guard flags");
  if (!ctx || !scalars || !bases || !err_inout || !guards_out5 || !nd || nd > MAX_RESOLVE || !n_bases || n_bases > n_records || n_records > MAX_RESOLVE) return BH_ERR_INVALID_ARG;
  if (group != BH_G1 && group != BH_G2) return BH_ERR_INVALID_ARG;
  // the strides msm_pick_sources hands the pass: dense, or G1 records 128 bytes apart
  if (group == BH_G1 ? (base_stride != 96 && base_stride != 128) : base_stride != 192) return BH_ERR_INVALID_ARG;
  if ((density_words != nullptr) != (word_prefix != nullptr) || skip >= ((size_t)1 << 31)) return BH_ERR_INVALID_ARG;
  if (!scalars_ok(scalars, fmt, nd)) return BH_ERR_INVALID_ARG;
  const size_t nwords = (nd + 63) / 64;
  const u32 lo_ref = err_resolve_lo_ref(ref_n ? ref_n : nd);   // as msm_finish: the job's own size unless it is a shard
  if (lo_ref >= 256) return BH_ERR_INVALID_ARG;

  Context &cx = ctx->c;
  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_scalars, d_density, d_prefix, d_bases, d_err;
  int rc;
  if ((rc = d_scalars.alloc(nd * 32, 0, st)) || (rc = d_scalars.upload(scalars, st)) ||
      (rc = d_bases.alloc(n_records * base_stride, 0, st)) || (rc = d_bases.upload(bases, st)) ||
      (rc = d_err.alloc(sizeof(ErrFlags), 0, st)) || (rc = d_err.upload(err_inout, st)))
    return rc;
  if (density_words &&
      ((rc = d_density.alloc(nwords * 8, 0, st)) || (rc = d_density.upload(density_words, st)) ||
       (rc = d_prefix.alloc((nwords + 1) * 4, 0, st)) || (rc = d_prefix.upload(word_prefix, st))))
    return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copies above may still be staged)
  const u64 *dens = density_words ? (const u64 *)d_density.p : nullptr;
  const u32 *prefix = density_words ? (const u32 *)d_prefix.p : nullptr;
  ErrFlags *err = (ErrFlags *)d_err.p;
  rc = group == BH_G1 ? launch_err_resolve<FpOps>(st, d_scalars.p, fmt, (u32)nd, dens, prefix, skip, n_bases, (const Affine<FpOps> *)d_bases.p, base_stride, lo_ref, err)
                      : launch_err_resolve<Fp2Ops>(st, d_scalars.p, fmt, (u32)nd, dens, prefix, skip, n_bases, (const Affine<Fp2Ops> *)d_bases.p, base_stride, lo_ref, err);
  if (rc) return rc;
  std::vector<unsigned char> g[R_WORDS];
  if ((rc = d_err.fetch(err_inout, g[R_ERR], st)) || (rc = d_scalars.fetch(nullptr, g[R_SCALARS], st)) || (rc = d_bases.fetch(nullptr, g[R_BASES], st)))
    return rc;
  if (density_words && ((rc = d_density.fetch(nullptr, g[R_DENSITY], st)) || (rc = d_prefix.fetch(nullptr, g[R_WORD_PREFIX], st)))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < R_WORDS; k++) guards_out5[k] = g[k].empty() ? 1u : guard_intact(g[k]);
  return BH_OK;
}
}  // extern "C"
