// libbellman_hip_test.so: stages 1 - 3 of a multiexp on their own - the density prefix, the recursive scan, the signed-digit
// recoding, the 8-bit sort of the classic plan, the fused recode-and-sort of the table plan and the zero-digit search - run by
// the shipped msm_run_stages over a plan of the shipped make_plan / make_table_plan; everything the kernels wrote comes back raw
// (bh_test_sort_* of include/bellman_hip_test.h; tests/test_gpu_sort_stage.py, tests/test_sort_stage_model_cpu.py).  This
// translation unit INCLUDES msm_stages.hip: the kernels, exclusive_scan_u32 and the static sizing functions are the shipped
// text, compiled a second time into the test library; the product library is built as before.  Every argument is validated
// on the host before anything is launched.  Every device buffer has its exact production element count - no rounding to 256
// bytes - and a guard behind it; buffers production takes unzeroed from the pool start filled with the sentinel byte.
#include <string.h>

#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_stages.hip"

namespace bh {
namespace sortstage {

constexpr size_t GUARD = 4096;                       // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;             // what the buffers production takes unzeroed from the pool hold here
constexpr u64 MAX_ENTRIES = (u64)1 << 21, MAX_SCAN = (u64)1 << 24;
enum { KIND_CLASSIC = 0, KIND_TABLE = 1 };
enum { PL_N, PL_C, PL_W, PL_ND, PL_WD, PL_NUM_TILES, PL_SORT_PASSES, PL_BASE_STRIDE, PL_PASS_BITS /* 4 */, PL_SPT = 12, PL_FIRST_TILES,
       PL_COUNTS, PL_SCAN_TMP, PL_SORT_TILE, PL_WIDE_TILE, PL_WIDE_THREADS, PL_SCAN_TILE, PL_GUARD, PL_SENTINEL, PL_ERR_BYTES, PL_WORDS };
enum { G_PAIRS_A, G_PAIRS_B, G_COUNTS, G_SCAN_TMP, G_ZSTART, G_WORD_PREFIX, G_ERR, G_SCALARS, G_WORDS };

// the conditions of msm_enqueue (32-bit pair positions, 31-bit base field) and the window sizes make_plan clamps to
static bool plan_args_ok(int kind, u64 n, u32 c, u64 stride) {
  if ((kind != KIND_CLASSIC && kind != KIND_TABLE) || !n || c < 2 || c > 24) return false;
  const u64 Wd = (256 + c - 1) / c;
  if (n >= ((u64)1 << 32) || Wd * n >= ((u64)1 << 32)) return false;
  if (kind == KIND_CLASSIC ? stride != 0 : (stride >= ((u64)1 << 31) || Wd * stride >= ((u64)1 << 31))) return false;
  return true;
}
static MsmPlan stage_plan(int kind, u64 n, u32 c, u64 stride, bool g2, int num_cus) {
  if (kind == KIND_CLASSIC) return make_plan(n, c, 8, g2);
  WindowTable t;
  t.c = c; t.W = (256 + c - 1) / c; t.stride = stride;
  return make_table_plan(n, t, 8, g2, num_cus);
}
static void plan_words(const MsmPlan &p, u64 *out) {
  memset(out, 0, PL_WORDS * sizeof(u64));
  out[PL_N] = p.n; out[PL_C] = p.c; out[PL_W] = p.W; out[PL_ND] = p.nd; out[PL_WD] = p.Wd; out[PL_NUM_TILES] = p.num_tiles;
  out[PL_SORT_PASSES] = p.sort_passes; out[PL_BASE_STRIDE] = p.base_stride;
  for (u32 pass = 0; pass < p.sort_passes && pass < 4; pass++) out[PL_PASS_BITS + pass] = p.W == 1 ? wide_pass_bits(p.c, pass) : 8;
  if (p.W == 1) { out[PL_SPT] = wide_scalars_per_tile(p.Wd); out[PL_FIRST_TILES] = wide_first_tiles(p); }
  out[PL_COUNTS] = sort_counts_elems(p);
  out[PL_SCAN_TMP] = scan_tmp_elems(out[PL_COUNTS] + 1);
  out[PL_SORT_TILE] = SORT_TILE; out[PL_WIDE_TILE] = WIDE_TILE; out[PL_WIDE_THREADS] = WIDE_THREADS; out[PL_SCAN_TILE] = SCAN_TILE;
  out[PL_GUARD] = GUARD; out[PL_SENTINEL] = SENTINEL; out[PL_ERR_BYTES] = sizeof(ErrFlags);
}

// a Montgomery scalar has to be a field element (< q): fe_from_mont is defined for those alone
static const u32 FR_MODULUS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
static bool below_modulus(const u32 *s) {
  for (int i = 7; i >= 0; i--)
    if (s[i] != FR_MODULUS[i]) return s[i] < FR_MODULUS[i];
  return false;
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
}  // namespace sortstage
}  // namespace bh

using namespace bh;
using namespace bh::sortstage;
extern "C" {
int bh_test_sort_plan(int kind, size_t n, unsigned c, size_t stride, int g2, int num_cus, uint64_t plan_out23[23]) {
  static_assert(PL_WORDS == 23, "include/bellman_hip_test.h documents 23 words");
  if (!plan_out23 || num_cus <= 0 || !plan_args_ok(kind, n, c, stride)) return BH_ERR_INVALID_ARG;
  plan_words(stage_plan(kind, n, c, stride, g2 != 0, num_cus), plan_out23);
  return BH_OK;
}
int bh_test_scan_dev(bh_ctx *ctx, uint32_t *data, size_t n, size_t *tmp_elems_out, uint32_t *tmp_out, uint32_t guards_out2[2]) {
  if (!tmp_elems_out || !n || n >= ((size_t)1 << 32)) return BH_ERR_INVALID_ARG;
  const size_t tmp_elems = scan_tmp_elems(n);
  *tmp_elems_out = tmp_elems;
  if (!data && !tmp_out && !guards_out2) return BH_OK;   // host only: the caller sizes tmp_out by it, then calls again
  if (!ctx || !data || !tmp_out || !guards_out2 || n > MAX_SCAN) return BH_ERR_INVALID_ARG;
  Context &cx = ctx->c;
  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_data, d_tmp;
  std::vector<unsigned char> g_data, g_tmp;
  int rc;
  if ((rc = d_data.alloc(n * 4, SENTINEL, st)) || (rc = d_tmp.alloc(tmp_elems * 4, SENTINEL, st)) || (rc = d_data.upload(data, st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copy above may still be staged)
  if ((rc = exclusive_scan_u32((u32 *)d_data.p, n, (u32 *)d_tmp.p, st))) return rc;
  if ((rc = d_data.fetch(data, g_data, st)) || (rc = d_tmp.fetch(tmp_out, g_tmp, st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  guards_out2[0] = guard_intact(g_data);
  guards_out2[1] = guard_intact(g_tmp);
  return BH_OK;
}
int bh_test_sort_stage_dev(bh_ctx *ctx, int kind, unsigned c, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                           size_t skip, size_t n_bases, size_t stride, uint64_t *pairs_a_out, uint64_t *pairs_b_out,
                           int *sorted_is_b_out, uint32_t *zstart_out, uint32_t *counts_out, uint32_t *word_prefix_out, void *err_out,
                           uint32_t guards_out8[8]) {
  static_assert(G_WORDS == 8, "include/bellman_hip_test.h documents 8 guard flags");
  if (!ctx || !scalars || !pairs_a_out || !pairs_b_out || !sorted_is_b_out || !zstart_out || !counts_out || !err_out || !guards_out8)
    return BH_ERR_INVALID_ARG;
  if (fmt != BH_SCALARS_CANONICAL && fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  if (!plan_args_ok(kind, nd, c, stride) || n_bases >= ((size_t)1 << 31) || skip >= ((size_t)1 << 31)) return BH_ERR_INVALID_ARG;
  if ((density_words != nullptr) != (word_prefix_out != nullptr)) return BH_ERR_INVALID_ARG;
  Context &cx = ctx->c;
  const MsmPlan p = stage_plan(kind, nd, c, stride, false, cx.num_cus);
  const u64 npairs = (u64)p.Wd * nd, nwords = ((u64)nd + 63) / 64;
  if (npairs > MAX_ENTRIES || p.c != c || p.nd != nd || (u64)p.W * p.n != npairs) return BH_ERR_INVALID_ARG;
  if (fmt == BH_SCALARS_MONT)
    for (size_t i = 0; i < nd; i++)
      if (!below_modulus((const u32 *)scalars + 8 * i)) return BH_ERR_INVALID_ARG;
  const u64 ncounts = sort_counts_elems(p);
  const size_t scan_elems = scan_tmp_elems(ncounts + 1);
  // the density prefix is scanned in the scratch that is sized for the counts (msm_enqueue)
  if (density_words && scan_tmp_elems(nwords) > scan_elems) return BH_ERR_INVALID_ARG;

  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_scalars, d_density, d_err, d_a, d_b, d_counts, d_scan, d_z, d_prefix;
  int rc;
  if ((rc = d_scalars.alloc((size_t)nd * 32, 0, st)) || (rc = d_scalars.upload(scalars, st)) ||
      // zeroed, as in production: the status words
      (rc = d_err.alloc(sizeof(ErrFlags), 0, st)) ||
      // from the pool, not zeroed
      (rc = d_a.alloc(npairs * 8, SENTINEL, st)) || (rc = d_b.alloc(npairs * 8, SENTINEL, st)) ||
      (rc = d_counts.alloc((ncounts + 1) * 4, SENTINEL, st)) || (rc = d_scan.alloc(scan_elems * 4, SENTINEL, st)) ||
      (rc = d_z.alloc((size_t)p.W * 4, SENTINEL, st)))
    return rc;
  if (density_words &&
      ((rc = d_density.alloc(nwords * 8, 0, st)) || (rc = d_density.upload(density_words, st)) || (rc = d_prefix.alloc((nwords + 1) * 4, SENTINEL, st))))
    return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copies above may still be staged)
  MsmBuffers b;
  b.pairs_a = (u64 *)d_a.p; b.pairs_b = (u64 *)d_b.p;
  b.counts = (u32 *)d_counts.p; b.scan_tmp = (u32 *)d_scan.p; b.zstart = (u32 *)d_z.p;
  b.word_prefix = density_words ? (u32 *)d_prefix.p : nullptr;
  b.err = (ErrFlags *)d_err.p;
  const u64 *sorted = nullptr;
  if ((rc = msm_run_stages(p, b, d_scalars.p, fmt, density_words ? (const u64 *)d_density.p : nullptr, skip, n_bases, st, &sorted))) return rc;
  if (sorted != b.pairs_a && sorted != b.pairs_b) return BH_ERR_HIP;
  *sorted_is_b_out = sorted == b.pairs_b;
  std::vector<unsigned char> g[G_WORDS];
  if ((rc = d_a.fetch(pairs_a_out, g[G_PAIRS_A], st)) || (rc = d_b.fetch(pairs_b_out, g[G_PAIRS_B], st)) ||
      (rc = d_counts.fetch(counts_out, g[G_COUNTS], st)) || (rc = d_scan.fetch(nullptr, g[G_SCAN_TMP], st)) ||
      (rc = d_z.fetch(zstart_out, g[G_ZSTART], st)) || (rc = d_err.fetch(err_out, g[G_ERR], st)) ||
      (rc = d_scalars.fetch(nullptr, g[G_SCALARS], st)))
    return rc;
  if (density_words && (rc = d_prefix.fetch(word_prefix_out, g[G_WORD_PREFIX], st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < G_WORDS; k++) guards_out8[k] = g[k].empty() ? 1u : guard_intact(g[k]);
  return BH_OK;
}
}  // extern "C"
