// Base vectors: entry points of include/bellman_hip.h that register, read, validate, compare and write them, the
// kernels of the uncompressed point codec, and the policy for their automatic window tables.
#include <string.h>

#include "bases_compare.cuh"
#include "handles.hpp"
#include "point_ops.hpp"
#include "points.hpp"

namespace bh {
// packs strided host records (optionally with an `infinity` flag byte) into dense device records
__global__ void pack_bases_kernel(const unsigned char *raw, size_t stride, long inf_offset, u32 rec_words,
                                  u32 *out, u64 n) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char *src = raw + i * stride;
  const bool inf = inf_offset >= 0 && src[inf_offset] != 0;
  for (u32 w = 0; w < rec_words; w++) {
    u32 v = 0;
    if (!inf) v = (u32)src[4 * w] | ((u32)src[4 * w + 1] << 8) | ((u32)src[4 * w + 2] << 16) | ((u32)src[4 * w + 3] << 24);
    out[i * rec_words + w] = v;
  }
}

// Zcash uncompressed encoding -> device records: one thread per 48-byte big-endian coordinate.
// coordinate order in: G1 x|y ; G2 x.c1|x.c0|y.c1|y.c0   out: G1 x|y ; G2 x.c0|x.c1|y.c0|y.c1
// `status` (optional, one word per point, zeroed by the caller) receives the PointStatus bits of the
// encoding rules of from_uncompressed_unchecked; `bad_flag` (optional) is the legacy any-compressed flag.
__global__ void decode_uncompressed_kernel(const unsigned char *raw, u32 coords_per_point, fp_t *out, u64 n,
                                           u32 *bad_flag, u32 *status) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * coords_per_point) return;
  const u64 pt = t / coords_per_point;
  const u32 ci = (u32)(t % coords_per_point);
  const unsigned char *p0 = raw + pt * coords_per_point * 48;
  const unsigned char flags = p0[0];
  if ((flags & 0x80) && bad_flag) atomicOr(bad_flag, 1u);   // compressed form is not this entry point's format
  const bool inf = (flags & 0x40) != 0;
  const unsigned char *src = p0 + (size_t)ci * 48;
  fp_t v;
  u32 nonzero = 0;
#pragma unroll
  for (int w = 0; w < 12; w++) {   // limb w (little-endian) = bytes [44-4w, 48-4w) big-endian
    const unsigned char *b = src + 44 - 4 * w;
    u32 x = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
    if (ci == 0 && w == 11) x &= 0x1fffffffu;   // strip the three flag bits
    nonzero |= x;
    v.l[w] = inf ? 0u : x;
  }
  if (status) {
    u32 st = 0;
    if (ci == 0) {
      if (flags & 0x80) st |= PT_COMPRESSED;
      if (flags & 0x20) st |= PT_SORT;
      if (inf) st |= PT_IS_INF;
    }
    if (inf && nonzero) st |= PT_INF_NONZERO;
    // canonical coordinate: value < p  (Fp::from_bytes)
    u32 borrow = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) (void)subb(v.l[w], FpParams::mod(w), borrow, borrow);
    if (!borrow) st |= PT_RANGE;
    if (st) atomicOr(status + pt, st);
  }
  if (!inf) fe_to_mont(v, v);
  // G2 stores c1 before c0 on the wire
  const u32 co = (coords_per_point == 4) ? (ci ^ 1u) : ci;
  out[pt * coords_per_point + co] = v;
}

// the inverse: Montgomery records -> the uncompressed encoding (Parameters::write, groth16/src/lib.rs:258-287 through
// bls12_381's to_uncompressed): one thread per coordinate; an all-zero record is the identity (flag 0x40, zeros)
__global__ void encode_uncompressed_kernel(const fp_t *pts, u32 coords_per_point, unsigned char *raw, u64 n) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * coords_per_point) return;
  const u64 pt = t / coords_per_point;
  const u32 ci = (u32)(t % coords_per_point);          // position on the wire
  const fp_t *rec = pts + pt * coords_per_point;
  u32 any = 0;
  for (u32 k = 0; k < coords_per_point; k++)
#pragma unroll
    for (int w = 0; w < 12; w++) any |= rec[k].l[w];
  const u32 co = (coords_per_point == 4) ? (ci ^ 1u) : ci;   // G2 stores c1 before c0 on the wire
  fp_t v = rec[co], c;
  fe_from_mont(c, v);
  u32 *dst = reinterpret_cast<u32 *>(raw + pt * coords_per_point * 48 + (size_t)ci * 48);
#pragma unroll
  for (int w = 0; w < 12; w++) {
    u32 x = any ? __builtin_bswap32(c.l[11 - w]) : 0u;
    if (!any && ci == 0 && w == 0) x = 0x40u;   // first byte of the record: the infinity flag
    dst[w] = x;
  }
}

// smallest index whose status makes Parameters::read fail (lib.rs:300-315)
__global__ void first_bad_point_kernel(const u32 *status, u64 n, u32 forbid_identity, unsigned long long *min_idx) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const u32 st = status[i];
    if ((st & PT_INVALID_MASK) || (forbid_identity && (st & PT_IS_INF))) atomicMin(min_idx, (unsigned long long)i);
  }
}
}  // namespace bh

using namespace bh;

// registers the finished device vector: mirrors its leading records on the host (ordered after whatever filled
// the vector on the context stream)
static int finish_bases(bh_ctx *ctx, bh_bases *b) {
  const size_t rec = b->group == BH_G1 ? 96 : 192;
  const size_t k = b->n < HOST_PREFIX_POINTS ? b->n : HOST_PREFIX_POINTS;
  b->host_prefix.resize(k * rec);
  if (k) {
    BH_HIP_CHECK(hipMemcpyAsync(b->host_prefix.data(), b->dev, k * rec, hipMemcpyDeviceToHost, ctx->c.stream));
    BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  }
  return BH_OK;
}
// Base vectors of up to 2^24 (G1) / 2^22 (G2) points get their window table at registration (BELLMAN_HIP_TABLE_MAX_LOG2
// overrides both limits, BELLMAN_HIP_TABLE_MAX_LOG2_G1 the G1 limit alone; 0 = never): a multiexp over a few thousand
// terms is a chain of latency-bound steps, and with the table the chain loses the 255-step doubling ladder over the
// windows and all but one of its bucket reductions (the CRS is registered once per circuit).
// G1 history: 2^16 until round 4; 2^18 after profiles/archive/r4_call13_fft_batched_loads_and_plan_sweeps.txt (2^17 1.04 vs
// 1.31 ms, 2^18 1.47 vs 1.72).  2^19 ... 2^22 were measured and NOT adopted (profiles/archive/r4_call16_g1_tables_2p19_2p22.txt,
// r4_call17_g1_tables_in_proofs.txt): a multiexp called alone gets faster - the classic plan ends in a HOST tail of 256
// doublings + 256 additions (16 windows x 16 bit sums, 0.27-0.44 ms by box), the table plan in 19 + 20: wall 2.21 vs
// 2.67 ms at 2^19, 3.92-3.95 vs 4.09-4.28 at 2^20, 6.95 vs 7.42 at 2^21, 12.3 vs 13.5 at 2^22 - but its bucket
// accumulation is slower per addition (2.89-2.94 vs 2.54-2.57 ms at 2^20: the same 16 n gathers come from a 2 GB table
// in HBM instead of a 128 MB vector in the Infinity Cache), and wherever the host tail is hidden behind the next job
// that is all that counts: two multiexps in flight 265 vs 282 M terms/s, a 2^20 proof 77.8 vs 74.9 ms (GPU part 23.6 vs
// 20.7), twelve proof threads 37-40 vs 43-45 proofs/s.  A caller whose multiexps run one at a time can opt in with
// BELLMAN_HIP_TABLE_MAX_LOG2_G1=22 (or bh_bases_precompute).
static unsigned auto_table_max_log2(int group) {
  const int v = env().table_max_log2, v1 = env().table_max_log2_g1;
  if (group == BH_G1 && v1 >= 0) return (unsigned)v1;
  // [r6] G1: up to 2^24 points (it was 2^18): a 13-row table at a 128-byte stride is 1.7 GB per 2^20 points, built in 0.13 s;
  // 2^23 24.6 -> 21.4 ms, 2^24 44.6 -> 40.5 (profiles/r6_call44_g1_tables_2p23_2p24.txt).  Always within the context's table
  // budget (a quarter of the memory by default): two of the 28 GB tables of 2^24-point queries fit, the next query stays classic
  return v >= 0 ? (unsigned)v : (group == BH_G1 ? 24u : 22u);
}
// G1 tables of 2^19 points and more are built at a 128-byte record stride (bh_bases::table_stride);
// BELLMAN_HIP_TABLE_PAD=0 keeps them dense
static bool table_will_pad(const bh_bases *b) {
  return env().table_pad && b->group == BH_G1 && b->n >= ((size_t)1 << 19);
}
static int new_bases(bh_ctx *ctx, int group, void *dev, size_t n, bool owned, bh_bases **out) {
  bh_bases *b = new bh_bases{group, dev, n, owned};
  b->ctx = ctx;
  // A wrapped (non-owned) buffer is a LIVE view: the caller may fill or rewrite it after wrapping, on any stream.
  // Nothing is snapshotted from it - no host mirror of the leading records (tiny multiexps take the kernel
  // pipeline), no automatic window table - so every multiexp reads the buffer as it is when the job runs.
  // (bh_bases_precompute on such a handle is an explicit snapshot, documented in the header.)
  if (!owned) { *out = b; return BH_OK; }
  int rc = finish_bases(ctx, b);
  if (rc != BH_OK) {
    if (dev) (void)hipFree(dev);
    delete b;
    return rc;
  }
  // automatic window table: only while all automatic tables of the context stay within its budget (default a
  // quarter of the device's memory, BELLMAN_HIP_TABLE_BUDGET_MB / bh_ctx_set_limits): a table is 13-32 x its base
  // vector (2^22 G2 points: 12.9 GB) and must not starve the per-proof workspaces
  const unsigned lg_table = auto_table_max_log2(group);
  const bool table_size = lg_table && n > TINY_MSM_MAX && n <= (size_t(1) << lg_table);   // (takes a window table instead)
  if (table_size) {
    // what the table takes at the stride it is built at - also the peak while it is built: bh_bases_precompute makes this
    // one allocation and nothing else
    const u32 c = table_window_bits(n, group == BH_G2);
    const size_t need = (size_t)((256 + c - 1) / c) * n * (table_will_pad(b) ? 128u : dense_rec_bytes(group));
    bool fits;
    {
      std::lock_guard<std::mutex> g(ctx->c.job_mu);
      fits = ctx->c.table_bytes + need <= ctx->c.table_budget;
      if (fits) ctx->c.table_bytes += need;   // reserved
    }
    if (fits) {
      if (bh_bases_precompute(ctx, b, 0) == BH_OK) {   // best effort
        b->auto_table = true;
        std::lock_guard<std::mutex> g(ctx->c.job_mu);
        ctx->c.tables.push_back(b);
        const size_t actual = table_bytes(b);   // (dense after all, if the table did not fit at the 128-byte stride)
        if (actual < need) ctx->c.table_bytes -= need - actual;
      } else {
        std::lock_guard<std::mutex> g(ctx->c.job_mu);
        ctx->c.table_bytes -= need;
      }
    }
  }
  // (a vector that got its window table gathers from the table; one that did not - too large, or over the table budget - gets the
  // 128-byte-stride copy of its points for the classic plan's gathers)
  if (group == BH_G1 && !b->table && n >= ((size_t)1 << 17) && n < ((size_t)1 << 31) &&
      (ctx->c.hbm_total == 0 || n * 128 <= ctx->c.hbm_total / 16)) {
    if (hipMalloc(&b->padded, n * 128) == hipSuccess) {
      if (hipMemcpy2DAsync(b->padded, 128, dev, 96, 96, n, hipMemcpyDeviceToDevice, ctx->c.stream) != hipSuccess ||
          hipStreamSynchronize(ctx->c.stream) != hipSuccess) {
        (void)hipFree(b->padded);
        b->padded = nullptr;
      }
    } else {
      (void)hipGetLastError();
      b->padded = nullptr;
    }
  }
  *out = b;
  return BH_OK;
}

extern "C" {

// ---- bases -------------------------------------------------------------------------------------
int bh_bases_register(bh_ctx *ctx, int group, const void *host_points, size_t n, size_t stride, long inf_offset,
                      bh_bases **out) {
  if (group != BH_G1 && group != BH_G2) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192;
  if (stride < rec) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev;
  BH_HIP_CHECK(hipMalloc(&dev.p, n ? n * rec : 16));
  if (n) {
    if (stride == rec && inf_offset < 0) {
      BH_HIP_CHECK(hipMemcpyAsync(dev.p, host_points, n * rec, hipMemcpyHostToDevice, ctx->c.stream));
    } else {
      DevGuard raw;
      BH_HIP_CHECK(hipMalloc(&raw.p, n * stride));
      BH_HIP_CHECK(hipMemcpyAsync(raw.p, host_points, n * stride, hipMemcpyHostToDevice, ctx->c.stream));
      hipLaunchKernelGGL(pack_bases_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->c.stream,
                         (const unsigned char *)raw.p, stride, inf_offset, (u32)(rec / 4), (u32 *)dev.p, (u64)n);
      BH_HIP_CHECK(hipGetLastError());
      BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
    }
    BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  }
  return new_bases(ctx, group, dev.release(), n, true, out);
}
int bh_bases_register_uncompressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n, bh_bases **out) {
  if (group != BH_G1 && group != BH_G2) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192;
  const u32 cpp = group == BH_G1 ? 2 : 4;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev, raw;
  BH_HIP_CHECK(hipMalloc(&dev.p, n ? n * rec : 16));
  if (n) {
    BH_HIP_CHECK(hipMalloc(&raw.p, n * rec + 4));
    u32 *flag = (u32 *)((char *)raw.p + n * rec);
    BH_HIP_CHECK(hipMemcpyAsync(raw.p, host_bytes, n * rec, hipMemcpyHostToDevice, ctx->c.stream));
    BH_HIP_CHECK(hipMemsetAsync(flag, 0, 4, ctx->c.stream));
    const u64 threads = (u64)n * cpp;
    hipLaunchKernelGGL(decode_uncompressed_kernel, dim3((u32)((threads + 255) / 256)), dim3(256), 0, ctx->c.stream,
                       (const unsigned char *)raw.p, cpp, (fp_t *)dev.p, (u64)n, flag, (u32 *)nullptr);
    BH_HIP_CHECK(hipGetLastError());
    u32 bad = 0;
    BH_HIP_CHECK(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, ctx->c.stream));
    BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
    if (bad) return BH_ERR_INVALID_ARG;
  }
  return new_bases(ctx, group, dev.release(), n, true, out);
}
int bh_bases_read_uncompressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n, unsigned flags,
                               bh_bases **out, size_t *bad_index) {
  if (!ctx || !out || (group != BH_G1 && group != BH_G2) || (n && !host_bytes)) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192;
  const u32 cpp = group == BH_G1 ? 2 : 4;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev;
  BH_HIP_CHECK(hipMalloc(&dev.p, n ? n * rec : 16));
  if (n) {
    hipStream_t st = ctx->c.stream;
    DevGuard raw;
    const size_t status_off = (n * rec + 15) & ~size_t(15);
    BH_HIP_CHECK(hipMalloc(&raw.p, status_off + n * 4 + 16));
    u32 *status = (u32 *)((char *)raw.p + status_off);
    unsigned long long *min_idx = (unsigned long long *)((char *)status + ((n * 4 + 7) & ~size_t(7)));
    unsigned long long first = ~0ULL;
    u32 first_status = 0;
    BH_HIP_CHECK(hipMemcpyAsync(raw.p, host_bytes, n * rec, hipMemcpyHostToDevice, st));
    BH_HIP_CHECK(hipMemsetAsync(status, 0, n * 4, st));
    BH_HIP_CHECK(hipMemsetAsync(min_idx, 0xff, 8, st));
    const u64 threads = (u64)n * cpp;
    hipLaunchKernelGGL(decode_uncompressed_kernel, dim3((u32)((threads + 255) / 256)), dim3(256), 0, st,
                       (const unsigned char *)raw.p, cpp, (fp_t *)dev.p, (u64)n, (u32 *)nullptr, status);
    BH_HIP_CHECK(hipGetLastError());
    if (flags & BH_POINTS_CHECKED) {
      int r = points_check(group, dev.p, n, status, st);
      if (r != BH_OK) { (void)hipStreamSynchronize(st); return r; }
    }
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(first_bad_point_kernel, dim3((u32)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, status,
                       (u64)n, (flags & BH_POINTS_FORBID_IDENTITY) ? 1u : 0u, min_idx);
    BH_HIP_CHECK(hipGetLastError());
    BH_HIP_CHECK(hipMemcpyAsync(&first, min_idx, 8, hipMemcpyDeviceToHost, st));
    BH_HIP_CHECK(hipStreamSynchronize(st));
    if (first != ~0ULL) {
      BH_HIP_CHECK(hipMemcpyAsync(&first_status, status + first, 4, hipMemcpyDeviceToHost, st));
      BH_HIP_CHECK(hipStreamSynchronize(st));
      if (bad_index) *bad_index = (size_t)first;
      return (first_status & PT_INVALID_MASK) ? BH_ERR_INVALID_POINT : BH_ERR_POINT_AT_INFINITY;
    }
  }
  return new_bases(ctx, group, dev.release(), n, true, out);
}
// from_compressed / from_compressed_unchecked for n points (point_read.hip): the twin of bh_bases_read_uncompressed
int bh_bases_read_compressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n, unsigned flags, bh_bases **out,
                             size_t *bad_index) {
  if (!ctx || !out || (group != BH_G1 && group != BH_G2) || (n && !host_bytes)) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192, enc = rec / 2;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev;
  BH_HIP_CHECK(hipMalloc(&dev.p, n ? n * rec : 16));
  if (n) {
    hipStream_t st = ctx->c.stream;
    DevGuard raw;
    const size_t status_off = (n * enc + 15) & ~size_t(15);
    BH_HIP_CHECK(hipMalloc(&raw.p, status_off + n * 4 + 16));
    u32 *status = (u32 *)((char *)raw.p + status_off);
    unsigned long long *min_idx = (unsigned long long *)((char *)status + ((n * 4 + 7) & ~size_t(7)));
    unsigned long long first = ~0ULL;
    u32 first_status = 0;
    BH_HIP_CHECK(hipMemcpyAsync(raw.p, host_bytes, n * enc, hipMemcpyHostToDevice, st));
    BH_HIP_CHECK(hipMemsetAsync(min_idx, 0xff, 8, st));
    const ReadLayout lay = {enc, 0, 0, rec, 0, 0, 1, 1, 0, 0};
    int r = points_read_compressed(group, raw.p, dev.p, n, lay, (flags & BH_POINTS_CHECKED) != 0, status, st);
    if (r != BH_OK) { (void)hipStreamSynchronize(st); return r; }
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(first_bad_point_kernel, dim3((u32)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, status,
                       (u64)n, (flags & BH_POINTS_FORBID_IDENTITY) ? 1u : 0u, min_idx);
    BH_HIP_CHECK(hipGetLastError());
    BH_HIP_CHECK(hipMemcpyAsync(&first, min_idx, 8, hipMemcpyDeviceToHost, st));
    BH_HIP_CHECK(hipStreamSynchronize(st));
    if (first != ~0ULL) {
      BH_HIP_CHECK(hipMemcpyAsync(&first_status, status + first, 4, hipMemcpyDeviceToHost, st));
      BH_HIP_CHECK(hipStreamSynchronize(st));
      if (bad_index) *bad_index = (size_t)first;
      return (first_status & PT_INVALID_MASK) ? BH_ERR_INVALID_POINT : BH_ERR_POINT_AT_INFINITY;
    }
  }
  return new_bases(ctx, group, dev.release(), n, true, out);
}
// curve and subgroup tests over records [first, first + count) of a resident handle (point_read.hip validate_kernel),
// VALIDATE_CHUNK records at a time on a stream of its own; the first offending record in order decides the return code
int bh_bases_validate(bh_ctx *ctx, const bh_bases *b, size_t first, size_t count, unsigned flags, uint32_t *status_host,
                      size_t *bad_index) {
  if (!ctx || !b || first > b->n || count > b->n - first || (flags & ~(BH_POINTS_CHECKED | BH_POINTS_FORBID_IDENTITY)))
    return BH_ERR_INVALID_ARG;
  if (!count) return BH_OK;
  constexpr size_t VALIDATE_CHUNK = size_t(1) << 20;   // 4 MB of status words
  const size_t rec = b->group == BH_G1 ? 96 : 192;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t chunk = count < VALIDATE_CHUNK ? count : VALIDATE_CHUNK;
  u32 *status = (u32 *)ctx->c.pool.acquire(chunk * 4 + 16);
  if (!status) return BH_ERR_HIP;
  unsigned long long *min_idx = (unsigned long long *)((char *)status + ((chunk * 4 + 7) & ~size_t(7)));
  void *stream = nullptr;
  if (bh_stream_create(ctx, &stream) != BH_OK) {
    ctx->c.pool.release(status);
    return BH_ERR_HIP;
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = BH_OK, verdict = BH_OK;
  for (size_t off = 0; off < count && rc == BH_OK; off += chunk) {
    const size_t m = count - off < chunk ? count - off : chunk;
    unsigned long long bad = ~0ULL;
    u32 bad_status = 0;
    if (hipMemsetAsync(min_idx, 0xff, 8, st) != hipSuccess) rc = BH_ERR_HIP;
    if (rc == BH_OK)
      rc = points_validate(b->group, (const char *)b->dev + (first + off) * rec, m, (flags & BH_POINTS_CHECKED) != 0, status, st);
    if (rc == BH_OK) {
      const u64 blocks = (m + 255) / 256;
      (void)hipGetLastError();
      hipLaunchKernelGGL(first_bad_point_kernel, dim3((u32)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, status, (u64)m,
                         (flags & BH_POINTS_FORBID_IDENTITY) ? 1u : 0u, min_idx);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, min_idx, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
          (status_host && hipMemcpyAsync(status_host + off, status, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = BH_ERR_HIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
    if (rc == BH_OK && bad != ~0ULL && verdict == BH_OK) {
      if (hipMemcpyAsync(&bad_status, status + bad, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        rc = BH_ERR_HIP;
      } else {
        if (bad_index) *bad_index = off + (size_t)bad;
        verdict = (bad_status & PT_INVALID_MASK) ? BH_ERR_INVALID_POINT : BH_ERR_POINT_AT_INFINITY;
      }
    }
    if (verdict != BH_OK && !status_host) break;   // later chunks cannot hold an earlier record
  }
  (void)hipStreamSynchronize(st);
  bh_stream_destroy(ctx, stream);
  ctx->c.pool.release(status);
  return rc != BH_OK ? rc : verdict;
}
// the first record at which two resident ranges differ (bases_compare.cuh): one launch on a stream of its own
int bh_bases_first_difference(bh_ctx *ctx, const bh_bases *a, size_t first_a, const bh_bases *b, size_t first_b, size_t count,
                              size_t *index) {
  if (!ctx || !a || !b || !index || a->group != b->group || first_a > a->n || count > a->n - first_a || first_b > b->n ||
      count > b->n - first_b)
    return BH_ERR_INVALID_ARG;
  *index = 0;
  if (!count) return BH_OK;
  const size_t rec = a->group == BH_G1 ? 96 : 192;
  const char *pa = (const char *)a->dev + first_a * rec, *pb = (const char *)b->dev + first_b * rec;
  if (((uintptr_t)pa | (uintptr_t)pb) & 15) return BH_ERR_INVALID_ARG;   // (a wrapped buffer: the kernel loads 16-byte vectors)
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  unsigned long long *min_idx = (unsigned long long *)ctx->c.pool.acquire(8);
  if (!min_idx) return BH_ERR_HIP;
  void *stream = nullptr;
  if (bh_stream_create(ctx, &stream) != BH_OK) {
    ctx->c.pool.release(min_idx);
    return BH_ERR_HIP;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long found = ~0ULL;
  int rc = BH_OK;
  if (hipMemsetAsync(min_idx, 0xff, 8, st) != hipSuccess) rc = BH_ERR_HIP;
  if (rc == BH_OK) rc = launch_first_difference(st, a->group, pa, pb, (u64)count, min_idx);
  if (rc == BH_OK && hipMemcpyAsync(&found, min_idx, 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  bh_stream_destroy(ctx, stream);
  ctx->c.pool.release(min_idx);
  if (rc == BH_OK) *index = found < (unsigned long long)count ? (size_t)found : count;
  return rc;
}
int bh_bases_download(bh_ctx *ctx, const bh_bases *b, size_t first, size_t count, void *out_host) {
  if (!ctx || !b || first + count > b->n) return BH_ERR_INVALID_ARG;
  const size_t rec = b->group == BH_G1 ? 96 : 192;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (count) {
    BH_HIP_CHECK(hipMemcpyAsync(out_host, (const char *)b->dev + first * rec, count * rec, hipMemcpyDeviceToHost, ctx->c.stream));
    BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  }
  return BH_OK;
}
int bh_bases_write_uncompressed(bh_ctx *ctx, const bh_bases *b, size_t first, size_t count, void *out_host_bytes) {
  if (!ctx || !b || first + count > b->n || (count && !out_host_bytes)) return BH_ERR_INVALID_ARG;
  const size_t rec = b->group == BH_G1 ? 96 : 192;
  const u32 cpp = b->group == BH_G1 ? 2 : 4;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (!count) return BH_OK;
  void *raw = ctx->c.pool.acquire(count * rec);
  if (!raw) return BH_ERR_HIP;
  const u64 threads = (u64)count * cpp;
  hipLaunchKernelGGL(encode_uncompressed_kernel, dim3((u32)((threads + 255) / 256)), dim3(256), 0, ctx->c.stream,
                     (const fp_t *)((const char *)b->dev + first * rec), cpp, (unsigned char *)raw, (u64)count);
  int rc = hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  if (rc == BH_OK && hipMemcpyAsync(out_host_bytes, raw, count * rec, hipMemcpyDeviceToHost, ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(ctx->c.stream) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  ctx->c.pool.release(raw);
  return rc;
}
int bh_bases_copy_dev(bh_ctx *ctx, int group, const void *dev_points, size_t n, bh_bases **out) {
  if (!ctx || !out || (group != BH_G1 && group != BH_G2)) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev;
  BH_HIP_CHECK(hipMalloc(&dev.p, n ? n * rec : 16));
  if (n) {
    BH_HIP_CHECK(hipMemcpyAsync(dev.p, dev_points, n * rec, hipMemcpyDeviceToDevice, ctx->c.stream));
    BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  }
  return new_bases(ctx, group, dev.release(), n, true, out);
}
int bh_bases_copy_out_dev(bh_ctx *ctx, const bh_bases *b, int group, size_t first, size_t count, void *dst_dev, void *stream) {
  if (!ctx || !b || b->group != group || first > b->n || count > b->n - first || (count && !dst_dev)) return BH_ERR_INVALID_ARG;
  const size_t rec = group == BH_G1 ? 96 : 192;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (count)
    BH_HIP_CHECK(hipMemcpyAsync(dst_dev, (const char *)b->dev + first * rec, count * rec, hipMemcpyDeviceToDevice,
                                pick_stream(ctx, stream)));
  return BH_OK;
}
int bh_bases_wrap_dev(bh_ctx *ctx, int group, const void *dev_points, size_t n, bh_bases **out) {
  if (!ctx || !out || (group != BH_G1 && group != BH_G2)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return new_bases(ctx, group, const_cast<void *>(dev_points), n, false, out);
}
int bh_bases_precompute(bh_ctx *ctx, bh_bases *b, unsigned window_bits) {
  if (!ctx || !b) return BH_ERR_INVALID_ARG;
  if (b->auto_table && b->ctx) {   // replaced by an explicit table: no longer the context's to drop or to count
    std::lock_guard<std::mutex> g(b->ctx->c.job_mu);
    forget_auto_table(b);
  }
  if (b->table) { (void)hipFree(b->table); b->table = nullptr; }
  if (b->n == 0) return BH_OK;
  const u32 c = window_bits ? window_bits : table_window_bits(b->n, b->group == BH_G2);
  if (c < 2 || c > 24) return BH_ERR_INVALID_ARG;
  const u32 W = (256 + c - 1) / c;
  const u32 rec = dense_rec_bytes(b->group);
  if ((u64)W * b->n >= ((u64)1 << 31)) return BH_ERR_INVALID_ARG;   // table rows must fit the 31-bit base field
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  // ONE allocation, at the stride the table keeps (128 bytes: one cache line per gathered record), and the kernel writes
  // every row where it stays.  If that size cannot be had the table is built dense - it is the same table
  u32 stride = table_will_pad(b) ? 128u : rec;
  void *t = nullptr;
  while (hipMalloc(&t, (size_t)W * b->n * stride) != hipSuccess) {
    (void)hipGetLastError();
    t = nullptr;
    if (stride == rec) return BH_ERR_HIP;   // not enough HBM for the table: the caller keeps using the plain bases
    stride = rec;
  }
  hipStream_t st = ctx->c.stream;
  int rc = window_table(b->group, BaseView{b->dev, rec}, t, stride, b->n, c, W, st);
  if (rc == BH_OK && hipStreamSynchronize(st) != hipSuccess) rc = BH_ERR_HIP;
  if (rc != BH_OK) { (void)hipFree(t); return rc; }
  b->table = t;
  b->table_stride = stride;
  b->tab = WindowTable{c, W, (u64)b->n};
  return BH_OK;
}
int bh_bases_table_info(const bh_bases *b, unsigned *window_bits, unsigned *rows, size_t *bytes) {
  if (!b) return BH_ERR_INVALID_ARG;
  if (window_bits) *window_bits = b->table ? b->tab.c : 0;
  if (rows) *rows = b->table ? b->tab.W : 0;
  if (bytes) *bytes = table_bytes(b);
  return BH_OK;
}
void bh_bases_release(bh_ctx *ctx, bh_bases *b) {
  (void)ctx;
  if (!b) return;
  if (b->auto_table && b->ctx) {
    std::lock_guard<std::mutex> g(b->ctx->c.job_mu);
    forget_auto_table(b);
  }
  if (b->table) (void)hipFree(b->table);
  if (b->padded) (void)hipFree(b->padded);
  if (b->owned && b->dev) (void)hipFree(b->dev);
  delete b;
}
size_t bh_bases_len(const bh_bases *b) { return b->n; }

int bh_bases_scale_powers(bh_ctx *ctx, const bh_bases *in, const void *c_mont, const void *g_mont, bh_bases **out) {
  if (!ctx || !in || !c_mont || !g_mont || !out) return BH_ERR_INVALID_ARG;
  *out = nullptr;
  fr_t c, g, t;
  memcpy(&c, c_mont, sizeof c);
  memcpy(&g, g_mont, sizeof g);
  fe_from_mont(t, c);
  const bool c_zero = fe_is_zero(t);
  fe_from_mont(t, g);
  if (c_zero || fe_is_zero(t)) return BH_ERR_UNEXPECTED_IDENTITY;
  const size_t rec = in->group == BH_G1 ? 96 : 192;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  DevGuard dev;
  BH_HIP_CHECK(hipMalloc(&dev.p, in->n ? in->n * rec : 16));
  if (in->n) {
    void *st = nullptr;   // a stream of its own: concurrent with other work on the context
    int rc = bh_stream_create(ctx, &st);
    if (rc) return rc;
    rc = point_mul_powers(ctx->c, in->group, in->dev, dev.p, in->n, c, g, (hipStream_t)st);
    bh_stream_destroy(ctx, st);
    if (rc) return rc;
  }
  return new_bases(ctx, in->group, dev.release(), in->n, true, out);
}

}  // extern "C"
