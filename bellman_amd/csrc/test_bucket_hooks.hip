// libbellman_hip_test.so: stage 4 of a multiexp on its own - msm_accumulate_kernel, msm_merge_chunks_kernel and the tail
// (msm_merge_tail_kernel, or msm_merge_runs_kernel + msm_merge_long_kernel) over a sorted pair stream the caller chooses, through
// the functions msm_enqueue calls (launch_accumulate, launch_merges of msm_ec.cuh; merge_plan, merge_bounds of
// msm_stage_plans.hpp); everything the kernels wrote comes back raw (bh_test_bucket_stage_* of include/bellman_hip_test.h; tests/test_gpu_bucket_stage.py,
// tests/test_bucket_stage_model_cpu.py).  Every input is validated on the host before anything is launched: a stream that
// could make a kernel leave its buffers is refused.  Next to them: what the stage gathers from - msm_pick_sources on tagged
// views (bh_test_msm_sources, host only) and window_table_kernel into a sentinel-filled buffer (bh_test_window_table_dev).
#include <string.h>

#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_ec.cuh"

namespace bh {
namespace bucketstage {

constexpr size_t GUARD = 4096;                       // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;             // what the buffers production takes unzeroed from the pool hold here
constexpr u32 MAX_N = 1u << 20, MAX_W = 16, MAX_SLOTS = 1u << 20, MAX_C = 16;
enum { ACC_FORMS = 6, MERGE_FORMS = 6, RAW_G1 = 6, RAW_G2_K3 = 7, RAW_G2 = 8 };
enum { PL_WALK, PL_RUN_LANES, PL_RUNS_ON_PAIRS, PL_BIG_CHUNKS, PL_PIECE, PL_MAX_LONG, PL_MAX_BIG, PL_MAX_PIECES, PL_WORDS };
enum { OV_WALK, OV_RUN_LANES, OV_BIG_CHUNKS, OV_BLOCK_CAP, OV_WORDS };

constexpr bool is_pow2(u32 g) { return g && !(g & (g - 1)); }
constexpr int acc_group(int f) { return f < 2 ? 1 : 2; }
constexpr int merge_group(int f) { return f < 2 ? 1 : 2; }

// the bundle of a merge form, and whether the form puts the medium runs on the group's half-point worker
static bool merge_form_geom(int form, BundleGeom &g, bool &pairs) {
  pairs = false;
  switch (form) {
    case 0: g = bundle_geom<FpOps>(); return true;
    case 1: g = bundle_geom<FpOps>(); pairs = true; return true;
    case 2: g = bundle_geom<Fp2K3Ops>(); return true;
    case 3: g = bundle_geom<Fp2K3Ops>(); pairs = true; return true;
    case 4: case 5: g = bundle_geom<Fp2Ops>(); return true;
    // the plan query alone: a bundle's plan as msm_enqueue gets it, whichever worker it puts the medium runs on
    case RAW_G1: g = bundle_geom<FpOps>(); return true;
    case RAW_G2_K3: g = bundle_geom<Fp2K3Ops>(); return true;
    case RAW_G2: g = bundle_geom<Fp2Ops>(); return true;
    default: return false;
  }
}
// workers per wavefront of the kernels' two parts: the big pieces run on the half-point worker where the group has one
static u32 medium_per_wave(const BundleGeom &g, bool pairs) { return pairs ? g.half_per_wave : g.per_wave; }
static u32 big_per_wave(const BundleGeom &g) { return g.half_kind != WK_NONE ? g.half_per_wave : g.per_wave; }

static MsmPlan stage_plan(u32 W, u32 n, u32 c, u32 K, u32 chunks_per_window) {
  MsmPlan p{};
  p.n = n; p.c = c; p.W = W; p.nb = 1u << (c - 1); p.NB = W * p.nb;
  p.chunk = K; p.chunks_per_window = chunks_per_window;
  p.nd = n; p.Wd = W;
  return p;
}
// dev: the sizes a launch is allowed; the host-only plan query takes any plan msm_enqueue accepts
static bool plan_args_ok(int merge_form, u32 W, u32 n, u32 c, u32 K, u32 chunks_per_window, bool dev) {
  if (merge_form < 0 || merge_form >= (dev ? (int)MERGE_FORMS : RAW_G2 + 1)) return false;
  if (!W || W > 128 || !n || c < 2 || c > 24 || !K || !chunks_per_window || (u64)chunks_per_window * K < n) return false;
  if ((u64)W * chunks_per_window >= ((u64)1 << 32)) return false;
  if (dev && (W > MAX_W || n > MAX_N || c > MAX_C || (u64)W * chunks_per_window > MAX_SLOTS)) return false;
  // the two launches of one-lane G2 are what a set of at most 128 buckets runs, the fused kernel every larger one
  const u32 NB = W << (c - 1);
  if (merge_form == 4 && NB <= 128) return false;
  if (merge_form == 5 && NB > 128) return false;
  return true;
}
// the shipped merge_plan of the form's bundle, then the overrides, then the shipped bounds for what results
static bool stage_merge_plan(int merge_form, const MsmPlan &p, int num_cus, const u32 *ov, MergePlan &mp) {
  BundleGeom geom;
  bool pairs;
  if (!merge_form_geom(merge_form, geom, pairs) || num_cus <= 0) return false;
  mp = merge_plan(p, geom, num_cus);
  if (merge_form >= MERGE_FORMS) {
    pairs = mp.runs_on_pairs;
  } else if (merge_form < 4) {   // the form says which worker folds the medium runs; its G has to fit that worker
    if (pairs != mp.runs_on_pairs && !(ov && ov[OV_RUN_LANES])) mp.run_lanes = 8;
    mp.runs_on_pairs = pairs;
  }
  if (ov) {
    if (ov[OV_WALK]) mp.walk = ov[OV_WALK];
    if (ov[OV_RUN_LANES]) mp.run_lanes = ov[OV_RUN_LANES];
    if (ov[OV_BIG_CHUNKS]) mp.big_chunks = ov[OV_BIG_CHUNKS];
  }
  if (!is_pow2(mp.run_lanes) || mp.run_lanes < 8 || mp.run_lanes > medium_per_wave(geom, pairs)) return false;
  if (mp.big_chunks < mp.walk) return false;
  const MergeBounds mb = merge_bounds((u64)p.W * p.chunks_per_window, mp.walk, mp.big_chunks, mp.piece);
  mp.max_long = mb.max_long; mp.max_big = mb.max_big; mp.max_pieces = mb.max_pieces;
  return true;
}
static void plan_words(const MergePlan &mp, u32 *out) {
  out[PL_WALK] = mp.walk; out[PL_RUN_LANES] = mp.run_lanes; out[PL_RUNS_ON_PAIRS] = mp.runs_on_pairs ? 1u : 0u;
  out[PL_BIG_CHUNKS] = mp.big_chunks; out[PL_PIECE] = mp.piece;
  out[PL_MAX_LONG] = mp.max_long; out[PL_MAX_BIG] = mp.max_big; out[PL_MAX_PIECES] = mp.max_pieces;
}

// what the kernels index with: live digits non-decreasing in [1, 2^(c-1)], base indices inside the vector
static bool stream_ok(const u64 *pairs, const u32 *zstart, u32 W, u32 n, u32 c, size_t n_bases) {
  const u32 nb = 1u << (c - 1);
  for (u32 w = 0; w < W; w++) {
    const u32 z = zstart[w];
    if (z > n) return false;
    u32 prev = 1;
    for (u32 i = z; i < n; i++) {
      const u64 e = pairs[(size_t)w * n + i];
      const u32 d = (u32)(e >> 32), idx = (u32)e & 0x7fffffffu;
      if (d < prev || d > nb || idx >= n_bases) return false;
      prev = d;
    }
  }
  return true;
}

struct DevBuf {   // `bytes` of payload + GUARD, freed on scope exit
  char *p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t n, int fill, hipStream_t st) {
    bytes = n;
    BH_HIP_CHECK(hipMalloc((void **)&p, n + GUARD));
    BH_HIP_CHECK(hipMemsetAsync(p, fill, n, st));
    BH_HIP_CHECK(hipMemsetAsync(p + n, SENTINEL, GUARD, st));
    return BH_OK;
  }
  int fetch(void *host, hipStream_t st) const {
    BH_HIP_CHECK(hipMemcpyAsync(host, p, bytes + GUARD, hipMemcpyDeviceToHost, st));
    return BH_OK;
  }
};

template <class M>
static int run_accumulate(int acc_form, hipStream_t st, const MsmPlan &p, const u64 *sorted, const u32 *zstart, const void *bases,
                          u32 stride, void *pts, void *head, void *tail, ErrFlags *err) {
  typedef XYZZ<M> Pt;
  const Affine<M> *b = (const Affine<M> *)bases;
#define BH_ACC(F, LDS) return launch_accumulate<F>(st, p, LDS, sorted, zstart, b, stride, (Pt *)pts, (Pt *)head, (Pt *)tail, err)
  if constexpr (M::WORDS == 24) {
    switch (acc_form) {
      case 2: BH_ACC(Fp2Ops, true);
      case 3: BH_ACC(Fp2Ops, false);
      case 4: BH_ACC(Fp2K3Ops, false);
      default: BH_ACC(Fp2PairOps, false);
    }
  } else {
    BH_ACC(FpOps, acc_form == 1);
  }
#undef BH_ACC
}
template <class FR>
static int run_merges(hipStream_t st, const MsmPlan &p, const MergePlan &mp, int num_cus, u32 block_cap, const u64 *sorted,
                      const u32 *zstart, void *pts, void *head, void *tail, void *long_runs, void *big_runs, void *pieces,
                      ErrFlags *err) {
  typedef XYZZ<typename FR::Mem> Pt;
  return launch_merges<FR>(st, p, mp, num_cus, block_cap, sorted, zstart, (Pt *)pts, (Pt *)head, (Pt *)tail, (LongRun *)long_runs,
                           (BigRun *)big_runs, (Pt *)pieces, err);
}
}  // namespace bucketstage
}  // namespace bh

using namespace bh;
using namespace bh::bucketstage;
extern "C" {
int bh_test_bucket_stage_shape(int acc_form, int merge_form, size_t out12[12]) {
  BundleGeom geom;
  bool pairs;
  if (!out12 || acc_form < 0 || acc_form >= ACC_FORMS || merge_form >= MERGE_FORMS || !merge_form_geom(merge_form, geom, pairs)) return BH_ERR_INVALID_ARG;
  if (acc_group(acc_form) != merge_group(merge_form)) return BH_ERR_INVALID_ARG;
  const bool g1 = acc_group(acc_form) == 1;
  out12[0] = g1 ? sizeof(XYZZ<FpOps>) : sizeof(XYZZ<Fp2Ops>);
  out12[1] = g1 ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  out12[2] = geom.long_piece;
  out12[3] = medium_per_wave(geom, pairs);
  out12[4] = big_per_wave(geom);
  out12[5] = 8;                    // G: a power of two from 8 (merge_plan's sweep starts there) to the medium worker's wavefront
  out12[6] = medium_per_wave(geom, pairs);
  out12[7] = GUARD;
  out12[8] = sizeof(LongRun);
  out12[9] = sizeof(BigRun);
  out12[10] = sizeof(ErrFlags);
  out12[11] = SENTINEL;
  return BH_OK;
}
int bh_test_merge_plan(int merge_form, unsigned W, unsigned n, unsigned c, unsigned K, unsigned chunks_per_window, int num_cus,
                       const uint32_t *overrides4, uint32_t plan_out8[8]) {
  MergePlan mp;
  if (!plan_out8 || !plan_args_ok(merge_form, W, n, c, K, chunks_per_window, false)) return BH_ERR_INVALID_ARG;
  if (!stage_merge_plan(merge_form, stage_plan(W, n, c, K, chunks_per_window), num_cus, overrides4, mp)) return BH_ERR_INVALID_ARG;
  plan_words(mp, plan_out8);
  return BH_OK;
}
int bh_test_bucket_stage_dev(bh_ctx *ctx, int acc_form, int merge_form, const uint64_t *pairs, const uint32_t *zstart, unsigned W,
                             unsigned n, const void *bases, size_t n_bases, unsigned base_stride, unsigned c, unsigned K,
                             unsigned chunks_per_window, const uint32_t *overrides4, uint32_t plan_out8[8], void *pts_out,
                             void *head_out, void *tail_out, void *long_out, void *big_out, void *pieces_out, void *err_out) {
  size_t shape[12];
  if (!ctx || !plan_out8 || bh_test_bucket_stage_shape(acc_form, merge_form, shape) != BH_OK) return BH_ERR_INVALID_ARG;
  if (!plan_args_ok(merge_form, W, n, c, K, chunks_per_window, true)) return BH_ERR_INVALID_ARG;
  const MsmPlan p = stage_plan(W, n, c, K, chunks_per_window);
  Context &cx = ctx->c;
  MergePlan mp;
  if (!stage_merge_plan(merge_form, p, cx.num_cus, overrides4, mp)) return BH_ERR_INVALID_ARG;
  plan_words(mp, plan_out8);
  const bool query = !pts_out && !head_out && !tail_out && !long_out && !big_out && !pieces_out && !err_out;
  if (query) return BH_OK;   // the caller sizes its buffers by the plan, then calls again
  if (!pts_out || !head_out || !tail_out || !long_out || !big_out || !pieces_out || !err_out) return BH_ERR_INVALID_ARG;
  const size_t rec = shape[0], arec = shape[1];
  const bool g1 = acc_group(acc_form) == 1;
  // the record strides the accumulation is launched with: dense, or G1 records 128 bytes apart (one-lane, in registers)
  if (!pairs || !zstart || !bases || !n_bases || n_bases >= ((size_t)1 << 24)) return BH_ERR_INVALID_ARG;
  if (base_stride != arec && !(acc_form == 0 && base_stride == 128)) return BH_ERR_INVALID_ARG;
  if (!stream_ok(pairs, zstart, W, n, c, n_bases)) return BH_ERR_INVALID_ARG;
  const u32 block_cap = overrides4 ? overrides4[OV_BLOCK_CAP] : 0;
  if (block_cap > 4096) return BH_ERR_INVALID_ARG;

  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  const size_t nslots = (size_t)W * chunks_per_window;
  DevBuf d_pairs, d_z, d_bases, d_pts, d_head, d_tail, d_long, d_big, d_pieces, d_err;
  int rc;
  if ((rc = d_pairs.alloc((size_t)W * n * 8, 0, st)) || (rc = d_z.alloc((size_t)W * 4, 0, st)) ||
      (rc = d_bases.alloc(n_bases * base_stride, 0, st)) ||
      // zeroed, as in production: the status words and the buckets (all-zero XYZZ == identity)
      (rc = d_err.alloc(sizeof(ErrFlags), 0, st)) || (rc = d_pts.alloc((size_t)p.NB * rec, 0, st)) ||
      // from the pool, not zeroed
      (rc = d_head.alloc(nslots * rec, SENTINEL, st)) || (rc = d_tail.alloc(nslots * rec, SENTINEL, st)) ||
      (rc = d_long.alloc((size_t)mp.max_long * sizeof(LongRun), SENTINEL, st)) ||
      (rc = d_big.alloc((size_t)mp.max_big * sizeof(BigRun), SENTINEL, st)) ||
      (rc = d_pieces.alloc((size_t)mp.max_pieces * rec, SENTINEL, st)))
    return rc;
  BH_HIP_CHECK(hipMemcpyAsync(d_pairs.p, pairs, (size_t)W * n * 8, hipMemcpyHostToDevice, st));
  BH_HIP_CHECK(hipMemcpyAsync(d_z.p, zstart, (size_t)W * 4, hipMemcpyHostToDevice, st));
  BH_HIP_CHECK(hipMemcpyAsync(d_bases.p, bases, n_bases * base_stride, hipMemcpyHostToDevice, st));
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copies above may still be staged)
  const u64 *sorted = (const u64 *)d_pairs.p;
  const u32 *zs = (const u32 *)d_z.p;
  ErrFlags *err = (ErrFlags *)d_err.p;
  rc = g1 ? run_accumulate<FpOps::Mem>(acc_form, st, p, sorted, zs, d_bases.p, base_stride, d_pts.p, d_head.p, d_tail.p, err)
          : run_accumulate<Fp2Ops::Mem>(acc_form, st, p, sorted, zs, d_bases.p, base_stride, d_pts.p, d_head.p, d_tail.p, err);
  if (rc) return rc;
#define BH_MERGE(FR) run_merges<FR>(st, p, mp, cx.num_cus, block_cap, sorted, zs, d_pts.p, d_head.p, d_tail.p, d_long.p, d_big.p, d_pieces.p, err)
  rc = merge_form < 2 ? BH_MERGE(FpOps) : merge_form < 4 ? BH_MERGE(Fp2K3Ops) : BH_MERGE(Fp2Ops);
#undef BH_MERGE
  if (rc) return rc;
  if ((rc = d_pts.fetch(pts_out, st)) || (rc = d_head.fetch(head_out, st)) || (rc = d_tail.fetch(tail_out, st)) ||
      (rc = d_long.fetch(long_out, st)) || (rc = d_big.fetch(big_out, st)) || (rc = d_pieces.fetch(pieces_out, st)) ||
      (rc = d_err.fetch(err_out, st)))
    return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  return BH_OK;
}
int bh_test_msm_sources(int group, int table_kind, int has_padded, uint32_t flags, unsigned opts_c, unsigned tab_c, unsigned tab_W,
                        uint64_t tab_row_records, uint64_t n, int acc_form, uint32_t out6[6]) {
  if (!out6 || (group != BH_G1 && group != BH_G2) || table_kind < 0 || table_kind > 2 || acc_form < 0 || acc_form > 2) return BH_ERR_INVALID_ARG;
  static const char tag[3] = {0, 0, 0};   // the views' pointers: &tag[0] dense, &tag[1] the padded copy, &tag[2] the table
  const u32 rec = group == BH_G1 ? 96u : 192u;
  MsmBases b;
  b.dense = {&tag[0], rec};
  if (has_padded) b.padded = {&tag[1], 128u};
  if (table_kind) b.table = {&tag[2], table_kind == 2 ? 128u : rec};
  b.tab = WindowTable{tab_c, tab_W, tab_row_records};
  b.n = tab_row_records;
  MsmOpts o;
  o.c = opts_c; o.flags = flags;
  const MsmSources s = msm_pick_sources(b, o, n, group, (AccForm)acc_form);
  if (!s.valid) return BH_ERR_INVALID_ARG;
  out6[0] = s.use_table; out6[1] = (u32)((const char *)s.gather.ptr - tag); out6[2] = s.gather.stride;
  out6[3] = (u32)((const char *)s.resolve.ptr - tag); out6[4] = s.resolve.stride; out6[5] = s.small_path;
  return BH_OK;
}
int bh_test_window_table_dev(bh_ctx *ctx, int group, const void *points, size_t n, unsigned stride, unsigned c, void *table_out) {
  if (!ctx || !points || !table_out || !n || n > 4096 || c < 2 || c > 24) return BH_ERR_INVALID_ARG;
  const u32 rec = group == BH_G1 ? 96u : 192u;
  if ((group != BH_G1 && group != BH_G2) || (stride != rec && !(group == BH_G1 && stride == 128))) return BH_ERR_INVALID_ARG;
  const u32 W = (256 + c - 1) / c;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = ctx->c.stream;
  DevBuf d_src, d_tab;
  int rc;
  if ((rc = d_src.alloc(n * rec, 0, st)) || (rc = d_tab.alloc((size_t)W * n * stride, SENTINEL, st))) return rc;
  BH_HIP_CHECK(hipMemcpyAsync(d_src.p, points, n * rec, hipMemcpyHostToDevice, st));
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copy above may still be staged)
  const BaseView src = {d_src.p, rec};
  rc = group == BH_G1 ? window_table_t<FpOps>(src, d_tab.p, stride, n, c, W, st) : window_table_t<Fp2Ops>(src, d_tab.p, stride, n, c, W, st);
  if (rc || (rc = d_tab.fetch(table_out, st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  return BH_OK;
}
}  // extern "C"
