// libbellman_hip_test.so: stage 5 of a multiexp on its own - the row / column sums, their two-stage split, the bit sums and
// totals - over filled buckets the caller chooses, through the functions msm_enqueue calls (reduce_plan of msm_stage_plans.hpp,
// launch_reduce of msm_ec.cuh), and the host tail (msm_host_tail) over what they leave (bh_test_reduce_* and
// bh_test_msm_host_tail of include/bellman_hip_test.h; tests/test_gpu_reduce_stage.py, tests/test_reduce_stage_model_cpu.py).
// The plan query copies out the schedule reduce_plan returns - the one launch_reduce issues; the device hook checks that
// schedule against its buffers on the host before anything is launched.
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_ec.cuh"

namespace bh {
namespace reducestage {

constexpr size_t GUARD = 4096;                       // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;             // what the buffers production takes unzeroed from the pool hold here
constexpr u64 MAX_NB = (u64)1 << 22;
enum { FORM_G1, FORM_G2_K3, FORM_G2, FORMS };
enum { KIND_CLASSIC = 0, KIND_TABLE = 1 };
enum { PL_C, PL_W, PL_NB_WINDOW, PL_NB, PL_LO_BITS, PL_HI_BITS, PL_TWO_LEN, PL_WANT_PART, PL_ROWCOL, PL_PART, PL_BITS, PL_GUARD,
       PL_SENTINEL, PL_RECORD, PL_AFFINE, PL_NUM_CUS, PL_WORDS };
// a job: the 11 words of bh_test_sum_jobs_dev (offsets inside the job's buffers), then which buffers and its workgroups
enum { SJ_MODE, SJ_GROUPS, SJ_COUNT, SJ_INNER, SJ_STRIDE, SJ_ISTRIDE, SJ_GROUP_SHIFT, SJ_SPLITS, SJ_LANES, SJ_IN_OFF, SJ_OUT_OFF,
       SJ_IN_BUF, SJ_OUT_BUF, SJ_NBLOCKS, SJ_WORDS };
// a launch: worker kind (the forms of bh_test_sum_jobs_dev), wavefronts per workgroup, workgroups, then three jobs
enum { LA_KIND, LA_WAVES, LA_BLOCKS, LA_MAX_LANES, LA_JOBS, LA_WORDS = LA_JOBS + 3 * SJ_WORDS };

constexpr bool is_pow2(u32 g) { return g && !(g & (g - 1)); }

static bool args_ok(int form, int kind, u32 c) {
  return form >= 0 && form < FORMS && (kind == KIND_CLASSIC || kind == KIND_TABLE) && c >= 2 && c <= 24;
}
// the shipped planners; only c, W and the bucket counts matter from here on (1024 terms, a table 1024 records a row)
static MsmPlan stage_plan(int form, int kind, u32 c, int num_cus) {
  const bool g2 = form != FORM_G1;
  if (kind == KIND_CLASSIC) return make_plan(1024, c, 8, g2);
  WindowTable t;
  t.c = c; t.W = (256 + c - 1) / c; t.stride = 1024;
  return make_table_plan(1024, t, 8, g2, num_cus);
}
struct Stage {
  MsmPlan p;
  ReducePlan rp;
  size_t rec, arec;
  u64 elems[RB_BUFS];
  std::vector<u32> launches;
};
static int stage(int form, int kind, u32 c, int num_cus, Stage &s) {
  s.p = stage_plan(form, kind, c, num_cus);
  if (s.p.c != c || s.p.NB != (u64)s.p.W << (c - 1)) return BH_ERR_INVALID_ARG;
  const BundleGeom geom = form == FORM_G1 ? bundle_geom<FpOps>() : form == FORM_G2_K3 ? bundle_geom<Fp2K3Ops>() : bundle_geom<Fp2Ops>();
  s.rp = reduce_plan(s.p, geom, num_cus);
  if (s.rp.overflow) return BH_ERR_INVALID_ARG;
  s.rec = form == FORM_G1 ? sizeof(XYZZ<FpOps>) : sizeof(XYZZ<Fp2Ops>);
  s.arec = form == FORM_G1 ? sizeof(Affine<FpOps>) : sizeof(Affine<Fp2Ops>);
  s.elems[RB_PTS] = s.p.NB; s.elems[RB_ROWCOL] = s.rp.rowcol_elems; s.elems[RB_PART] = s.rp.part_elems; s.elems[RB_BITS] = s.rp.bits_elems;
  // the plan's schedule in the word layout of include/bellman_hip_test.h
  s.launches.assign((size_t)s.rp.n_launches * LA_WORDS, 0);
  for (u32 i = 0; i < s.rp.n_launches; i++) {
    const ReduceLaunch &l = s.rp.launch[i];
    u32 *w = s.launches.data() + (size_t)i * LA_WORDS;
    w[LA_KIND] = l.kind; w[LA_WAVES] = l.waves; w[LA_BLOCKS] = l.blocks;
    w[LA_MAX_LANES] = l.waves * (l.kind == geom.full_kind ? geom.per_wave : geom.half_per_wave);
    for (int q = 0; q < 3; q++) {
      const ReduceJob &j = l.j[q];
      u32 *sj = w + LA_JOBS + q * SJ_WORDS;
      sj[SJ_MODE] = j.d.mode; sj[SJ_GROUPS] = j.d.groups; sj[SJ_COUNT] = j.d.count; sj[SJ_INNER] = j.d.inner; sj[SJ_STRIDE] = j.d.stride;
      sj[SJ_ISTRIDE] = j.d.istride; sj[SJ_GROUP_SHIFT] = j.d.group_shift; sj[SJ_SPLITS] = j.d.splits; sj[SJ_LANES] = j.d.lanes;
      sj[SJ_NBLOCKS] = j.nblocks;
      if (!j.d.groups) { sj[SJ_IN_BUF] = sj[SJ_OUT_BUF] = 0xffffffffu; continue; }   // nothing to do: its buffers are never used
      if (j.in_off >= ((u64)1 << 32) || j.out_off >= ((u64)1 << 32)) return BH_ERR_INVALID_ARG;
      sj[SJ_IN_BUF] = j.in_buf; sj[SJ_IN_OFF] = (u32)j.in_off;
      sj[SJ_OUT_BUF] = j.out_buf; sj[SJ_OUT_OFF] = (u32)j.out_off;
    }
  }
  return BH_OK;
}
static void plan_words(const Stage &s, int num_cus, u32 *out) {
  out[PL_C] = s.p.c; out[PL_W] = s.p.W; out[PL_NB_WINDOW] = s.p.nb; out[PL_NB] = s.p.NB; out[PL_LO_BITS] = s.p.lo_bits;
  out[PL_HI_BITS] = s.p.hi_bits; out[PL_TWO_LEN] = s.rp.two_len; out[PL_WANT_PART] = s.rp.want_part ? 1u : 0u;
  out[PL_ROWCOL] = (u32)s.rp.rowcol_elems; out[PL_PART] = (u32)s.rp.part_elems; out[PL_BITS] = (u32)s.rp.bits_elems;
  out[PL_GUARD] = GUARD; out[PL_SENTINEL] = SENTINEL; out[PL_RECORD] = (u32)s.rec; out[PL_AFFINE] = (u32)s.arec;
  out[PL_NUM_CUS] = (u32)num_cus;
}
// every record a launch reads or writes lies inside the buffer it names, and its lane counts fit its workgroups
static bool launches_in_bounds(const Stage &s) {
  for (size_t at = 0; at + LA_WORDS <= s.launches.size(); at += LA_WORDS) {
    const u32 *l = s.launches.data() + at;
    for (int q = 0; q < 3; q++) {
      const u32 *w = l + LA_JOBS + q * SJ_WORDS;
      const u64 groups = w[SJ_GROUPS], count = w[SJ_COUNT], inner = w[SJ_INNER], splits = w[SJ_SPLITS];
      if (!groups) continue;
      if (w[SJ_IN_BUF] >= RB_BUFS || w[SJ_OUT_BUF] >= RB_BUFS || w[SJ_OUT_BUF] == RB_PTS || w[SJ_IN_BUF] == RB_BITS) return false;
      if (!count || !inner || !splits || count % splits || groups % splits || w[SJ_GROUP_SHIFT] > 24) return false;
      if (!is_pow2(w[SJ_LANES]) || w[SJ_LANES] > l[LA_MAX_LANES]) return false;
      if (w[SJ_OUT_OFF] + groups > s.elems[w[SJ_OUT_BUF]]) return false;
      const u64 outer_max = (groups / splits - 1) / inner;
      u64 last;
      if (w[SJ_MODE] == SUM_STRIDED) last = (inner - 1) * w[SJ_ISTRIDE] + (count - 1) * w[SJ_STRIDE];
      else if (w[SJ_MODE] == SUM_BITS && is_pow2((u32)count) && splits == 1 && ((u64)1 << inner) <= count) last = count - 1;
      else return false;
      if (w[SJ_IN_OFF] + (outer_max << w[SJ_GROUP_SHIFT]) + last >= s.elems[w[SJ_IN_BUF]]) return false;
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
    if (n) BH_HIP_CHECK(hipMemsetAsync(p, fill, n, st));
    BH_HIP_CHECK(hipMemsetAsync(p + n, SENTINEL, GUARD, st));
    return BH_OK;
  }
  // the payload into `host`, the guard into `guard`
  int fetch(void *host, unsigned char *guard, hipStream_t st) const {
    if (bytes) BH_HIP_CHECK(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, st));
    BH_HIP_CHECK(hipMemcpyAsync(guard, p + bytes, GUARD, hipMemcpyDeviceToHost, st));
    return BH_OK;
  }
};
static u32 guard_intact(const unsigned char *g) {
  for (size_t i = 0; i < GUARD; i++)
    if (g[i] != SENTINEL) return 0;
  return 1;
}
template <class FR>
static int run_reduce(hipStream_t st, const Stage &s, const void *pts, void *rowcol, void *part, void *bits) {
  typedef XYZZ<typename FR::Mem> Pt;
  return launch_reduce<FR>(st, s.rp, (const Pt *)pts, (Pt *)rowcol, s.rp.want_part ? (Pt *)part : nullptr, (Pt *)bits);
}
}  // namespace reducestage
}  // namespace bh

using namespace bh;
using namespace bh::reducestage;
extern "C" {
int bh_test_reduce_plan(bh_ctx *ctx, int form, int kind, unsigned c, int num_cus, uint32_t plan_out16[16], uint32_t *launches_out,
                        size_t max_launches, size_t *n_launches_out) {
  static_assert(PL_WORDS == 16 && LA_WORDS == 46 && SJ_WORDS == 14, "include/bellman_hip_test.h documents these counts");
  if (!plan_out16 || !n_launches_out || !args_ok(form, kind, c) || num_cus < 0 || (!num_cus && !ctx)) return BH_ERR_INVALID_ARG;
  if (!num_cus) num_cus = ctx->c.num_cus;
  Stage s;
  if (int rc = stage(form, kind, c, num_cus, s)) return rc;
  plan_words(s, num_cus, plan_out16);
  const size_t n = s.launches.size() / LA_WORDS;
  *n_launches_out = n;
  if (launches_out) {
    if (n > max_launches) return BH_ERR_INVALID_ARG;
    memcpy(launches_out, s.launches.data(), s.launches.size() * sizeof(u32));
  }
  return BH_OK;
}
int bh_test_reduce_stage_dev(bh_ctx *ctx, int form, int kind, unsigned c, int num_cus, const void *pts_in, void *rowcol_out,
                             void *part_out, void *bits_out, uint32_t guards_out4[4], void *affine_out) {
  if (!ctx || !pts_in || !rowcol_out || !part_out || !bits_out || !guards_out4 || !affine_out) return BH_ERR_INVALID_ARG;
  if (!args_ok(form, kind, c) || num_cus < 0) return BH_ERR_INVALID_ARG;
  Context &cx = ctx->c;
  if (!num_cus) num_cus = cx.num_cus;
  Stage s;
  if (int rc = stage(form, kind, c, num_cus, s)) return rc;
  if (s.p.NB > MAX_NB || !launches_in_bounds(s)) return BH_ERR_INVALID_ARG;

  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_pts, d_rowcol, d_part, d_bits;
  int rc;
  if ((rc = d_pts.alloc(s.elems[RB_PTS] * s.rec, 0, st)) ||
      // zeroed, as in production: the result slots
      (rc = d_bits.alloc(s.elems[RB_BITS] * s.rec, 0, st)) ||
      // from the pool, not zeroed
      (rc = d_rowcol.alloc(s.elems[RB_ROWCOL] * s.rec, SENTINEL, st)) || (rc = d_part.alloc(s.elems[RB_PART] * s.rec, SENTINEL, st)))
    return rc;
  BH_HIP_CHECK(hipMemcpyAsync(d_pts.p, pts_in, d_pts.bytes, hipMemcpyHostToDevice, st));
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copy above may still be staged)
  rc = form == FORM_G1      ? run_reduce<FpOps>(st, s, d_pts.p, d_rowcol.p, d_part.p, d_bits.p)
       : form == FORM_G2_K3 ? run_reduce<Fp2K3Ops>(st, s, d_pts.p, d_rowcol.p, d_part.p, d_bits.p)
                            : run_reduce<Fp2Ops>(st, s, d_pts.p, d_rowcol.p, d_part.p, d_bits.p);
  if (rc) return rc;
  std::vector<unsigned char> g(RB_BUFS * GUARD);
  std::vector<unsigned char> pts_back(d_pts.bytes);   // the buckets are read-only here: they have to come back as they went
  if ((rc = d_pts.fetch(pts_back.data(), g.data() + RB_PTS * GUARD, st)) || (rc = d_rowcol.fetch(rowcol_out, g.data() + RB_ROWCOL * GUARD, st)) ||
      (rc = d_part.fetch(part_out, g.data() + RB_PART * GUARD, st)) || (rc = d_bits.fetch(bits_out, g.data() + RB_BITS * GUARD, st)))
    return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < RB_BUFS; k++) guards_out4[k] = guard_intact(g.data() + (size_t)k * GUARD);
  if (memcmp(pts_back.data(), pts_in, d_pts.bytes) != 0) guards_out4[RB_PTS] = 0;
  // the shipped host tail over what the device left (as msm_finish: the records of `bits` in their device layout)
  if (form == FORM_G1) msm_host_tail<FpOps>(s.p, (const XYZZ<FpOps> *)bits_out, affine_out);
  else msm_host_tail<Fp2Ops>(s.p, (const XYZZ<Fp2Ops> *)bits_out, affine_out);
  return BH_OK;
}
int bh_test_msm_host_tail(int group, int kind, unsigned c, const void *bits_in, void *affine_out) {
  if ((group != 1 && group != 2) || !bits_in || !affine_out || !args_ok(FORM_G1, kind, c)) return BH_ERR_INVALID_ARG;
  const MsmPlan p = stage_plan(group == 1 ? FORM_G1 : FORM_G2, kind, c, 256);
  if (p.c != c) return BH_ERR_INVALID_ARG;
  if (group == 1) msm_host_tail<FpOps>(p, (const XYZZ<FpOps> *)bits_in, affine_out);
  else msm_host_tail<Fp2Ops>(p, (const XYZZ<Fp2Ops> *)bits_in, affine_out);
  return BH_OK;
}
}  // extern "C"
