// libbellman_hip_test.so: stages 1 - 3 of a MANY-JOB on their own (bh_test_many_stage_dev of include/bellman_hip_test.h;
// tests/test_gpu_msm_many.py) - the density prefix, msm_many_digits_kernel, the 8-bit sort of every bucket set and the
// zero-digit search, run by the shipped msm_run_stages over a plan of the shipped make_many_plan (the definitions are the
// shipped text that test_sort_hooks.hip compiles into this library).  Every argument is validated on the host before
// anything is launched.  Every device buffer has its exact production element count - no rounding to 256 bytes - and a
// guard behind it; buffers production takes unzeroed from the pool start filled with the sentinel byte.
#include <string.h>

#include <vector>

#include "../../include/bellman_hip_test.h"
#include "msm_types.hpp"

namespace bh {
namespace manystage {

constexpr size_t GUARD = 4096;             // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;   // what the buffers production takes unzeroed from the pool hold here
constexpr u64 MAX_ENTRIES = (u64)1 << 22;
enum { G_PAIRS_A, G_PAIRS_B, G_COUNTS, G_SCAN_TMP, G_ZSTART, G_WORD_PREFIX, G_ERR, G_SCALARS, G_WORDS };

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
}  // namespace manystage
}  // namespace bh

using namespace bh;
using namespace bh::manystage;
extern "C" int bh_test_many_stage_dev(bh_ctx *ctx, int table, unsigned c, const void *scalars, int fmt, size_t nd, size_t k,
                                      const uint64_t *density_words, size_t skip, size_t n_bases, size_t stride,
                                      uint64_t *sorted_out, uint32_t *zstart_out, void *err_out, uint32_t plan_out4[4],
                                      uint32_t guards_out8[8]) {
  static_assert(G_WORDS == 8, "include/bellman_hip_test.h documents 8 guard flags");
  if (!ctx || !scalars || !sorted_out || !zstart_out || !err_out || !plan_out4 || !guards_out8) return BH_ERR_INVALID_ARG;
  if (fmt != BH_SCALARS_CANONICAL && fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  if (!nd || k < 2 || k >= 65536 || c < 2 || c > 24 || nd >= ((size_t)1 << 31) || n_bases >= ((size_t)1 << 31) || skip >= ((size_t)1 << 31))
    return BH_ERR_INVALID_ARG;
  if (table ? (stride == 0 || stride >= ((size_t)1 << 31)) : stride != 0) return BH_ERR_INVALID_ARG;
  Context &cx = ctx->c;
  WindowTable t;
  t.c = c; t.W = (256 + c - 1) / c; t.stride = stride;
  const MsmPlan p = make_many_plan(nd, k, table ? &t : nullptr, c, 0, false, cx.num_cus);
  if (!many_plan_valid(p, n_bases) || p.c != c || p.nd != nd || p.vectors != k) return BH_ERR_INVALID_ARG;
  const u64 npairs = (u64)p.W * p.n, nwords = ((u64)nd + 63) / 64;
  if (npairs > MAX_ENTRIES || npairs != (u64)k * p.Wd * nd) return BH_ERR_INVALID_ARG;
  const u64 ncounts = sort_counts_elems(p);
  const size_t scan_elems = scan_tmp_elems(ncounts + 1);
  if (density_words && scan_tmp_elems(nwords) > scan_elems) return BH_ERR_INVALID_ARG;
  plan_out4[0] = p.W; plan_out4[1] = p.n; plan_out4[2] = p.sort_passes; plan_out4[3] = p.Wd;

  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  DevBuf d_scalars, d_density, d_err, d_a, d_b, d_counts, d_scan, d_z, d_prefix;
  int rc;
  if ((rc = d_scalars.alloc(k * nd * 32, 0, st)) || (rc = d_scalars.upload(scalars, st)) ||
      (rc = d_err.alloc(sizeof(ErrFlags), 0, st)) ||   // zeroed, as in production: the status words
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
  if ((rc = msm_run_stages(p, b, d_scalars.p, fmt, density_words ? (const u64 *)d_density.p : nullptr, skip, n_bases, st, &sorted,
                           (u64)nd * 32)))
    return rc;
  if (sorted != b.pairs_a && sorted != b.pairs_b) return BH_ERR_HIP;
  const bool is_b = sorted == b.pairs_b;
  std::vector<unsigned char> g[G_WORDS];
  if ((rc = d_a.fetch(is_b ? nullptr : sorted_out, g[G_PAIRS_A], st)) || (rc = d_b.fetch(is_b ? sorted_out : nullptr, g[G_PAIRS_B], st)) ||
      (rc = d_counts.fetch(nullptr, g[G_COUNTS], st)) || (rc = d_scan.fetch(nullptr, g[G_SCAN_TMP], st)) ||
      (rc = d_z.fetch(zstart_out, g[G_ZSTART], st)) || (rc = d_err.fetch(err_out, g[G_ERR], st)) ||
      (rc = d_scalars.fetch(nullptr, g[G_SCALARS], st)))
    return rc;
  if (density_words && (rc = d_prefix.fetch(nullptr, g[G_WORD_PREFIX], st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int q = 0; q < G_WORDS; q++) guards_out8[q] = g[q].empty() ? 1u : guard_intact(g[q]);
  return BH_OK;
}
