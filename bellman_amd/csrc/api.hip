// extern "C" surface of libbellman_hip (declared and documented in include/bellman_hip.h).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>

#include "../../include/bellman_hip.h"
#include "bases_compare.cuh"
#include "common.hpp"
#include "msm_types.hpp"
#include "shard_cuts.hpp"

namespace bh {
// fft.hip
int ntt_run(Context &c, fr_t *data, fr_t *scratch, uint32_t log_n, int mode, hipStream_t st);
int fr_mul_assign(Context &c, fr_t *a, const fr_t *b, u64 n, hipStream_t st);
int fr_sub_assign(Context &c, fr_t *a, const fr_t *b, u64 n, hipStream_t st);
int fr_divide_by_z(Context &c, fr_t *a, uint32_t log_n, hipStream_t st);
int fr_distribute_powers(Context &c, fr_t *a, u64 n, const fr_t &g, hipStream_t st);
int h_poly_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, fr_t *scratch, uint32_t log_n, hipStream_t st);
int fr_gen_powers(Context &c, fr_t *out, u64 n, const fr_t &g, const fr_t &scale, hipStream_t st);
int ntt_run_many(Context &c, fr_t *data, u64 stride, u64 k, uint32_t log_n, int mode, fr_t *scratch, u64 scratch_vectors, hipStream_t st);
int ntt_run_each(Context &c, fr_t *data, u64 stride, u64 k, uint32_t log_n, int mode, fr_t *scratch, hipStream_t st);
int h_poly_many_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, u64 stride, u64 k, uint32_t log_n, fr_t *scratch, u64 scratch_vectors,
                    hipStream_t st);
int h_poly_each_dev(Context &c, fr_t *a, fr_t *b, fr_t *cc, u64 stride, u64 k, uint32_t log_n, fr_t *scratch, hipStream_t st);
// point_fft.hip
int point_fft(Context &c, int group, void *pts, uint32_t log_n, int mode, hipStream_t st);
int point_distribute_powers(Context &c, int group, void *pts, u64 n, const fr_t &g, hipStream_t st);
int point_divide_by_z(int group, void *pts, uint32_t log_n, hipStream_t st);
int point_mul_assign(int group, void *pts, const void *scalars_mont, u64 n, hipStream_t st);
int point_sub_assign(int group, void *a, const void *b, u64 n, hipStream_t st);
// point_mul.hip
int point_mul_each(int group, const void *in, void *out, u64 n, const void *scalars, int fmt, hipStream_t st);
int point_mul_powers(Context &c, int group, const void *in, void *out, u64 n, const fr_t &cc, const fr_t &g, hipStream_t st);
// msm.hip
struct MsmJobImpl;
MsmJobImpl *msm_job_new(Context *ctx, int group);
void msm_job_delete(MsmJobImpl *j);
int msm_job_enqueue(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                    const u64 *density_dev, const MsmOpts &opts);
int msm_job_finish(MsmJobImpl &job, void *out_affine, float *ms, u64 *stats8 = nullptr);
int msm_job_finish_many(MsmJobImpl &job, void *out_affine_k, size_t k, float *ms, u64 *stats8, bool *fallback);
int msm_debug_stages(Context &c, const void *scalars_host, u64 n, int fmt, unsigned cbits, u64 *pairs_out, u32 *zstart_out);
void msm_job_track(MsmJobImpl &job);
int msm_job_start(MsmJobImpl &job);
bool msm_slot_try_reserve(Context &c);
void msm_slot_release(Context &c);
bool msm_complete_oldest(Context &c);
size_t msm_jobs_in_flight(Context &c);
hipStream_t msm_job_stream(MsmJobImpl &job);
int msm_job_after(MsmJobImpl &job, hipStream_t after);
void msm_job_set_result(MsmJobImpl &job, int rc, const void *affine_record);
void msm_job_own(MsmJobImpl &job, void *dev_ptr);
int fixed_base_mul(int group, const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev,
                   hipStream_t st, void *table_dev);
void host_point_add(int group, void *r, const void *a, const void *b, u64 n);
void host_point_mul(int group, void *r, const void *a, const void *k);
void host_point_lincomb(int group, void *r, const void *pts, const void *scalars, u64 n);

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

constexpr size_t HOST_PREFIX_POINTS = 64;   // leading records mirrored on the host for the tiny-multiexp path
constexpr size_t TINY_MSM_MAX = 8;          // multiexps of at most this many terms are answered on the host

struct bh_bases {
  int group;
  void *dev;
  size_t n;
  bool owned;
  // the first min(n, HOST_PREFIX_POINTS) records on the host: create_proof's `inputs` multiexps have one or
  // two terms (prover.rs:275-280,296-300,312-316) - a kernel pipeline for them is all launch latency
  std::vector<unsigned char> host_prefix = {};
  // optional window table (bh_bases_precompute): [W][n] affine records, row 0 = a copy of the bases
  void *table = nullptr;
  WindowTable tab = {0, 0, 0};
  bool auto_table = false;   // built at registration under the context's table budget; bh_ctx_trim may drop it
  bh_ctx *ctx = nullptr;
  // [r4] G1 vectors that run the classic plan (>= 2^17 points, owned by the handle): a second copy of the records at a
  // 128-byte stride, which is what the bucket accumulation gathers from - every gather is exactly one cache line (a
  // 96-byte record at a 96-byte stride straddles two lines half of the time).  profiles/archive/r4_call11_*.txt:
  // FETCH_SIZE of the accumulate launch 2.20 -> 1.58 GB at 2^20; accumulate -1 % at 2^20 (the table sits in the
  // Infinity Cache either way), -3 % at 2^22 (it does not).  Dense `dev` stays what every other path and the API see.
  // Vectors whose copy would exceed 1/16 of the device memory are not padded.
  void *padded = nullptr;
  // [r4] ... and the window table of a G1 vector too large for the Infinity Cache (>= 2^19 points: 16 rows of 2^19
  // records are 0.8 GB) is built and kept at that stride only (table_will_pad): `table` then holds W * n records 128 bytes
  // apart.  What a job reads from which of these three, and at what stride: msm_pick_sources (msm_types.hpp).
  u32 table_stride = 0;   // bytes between the records of `table`
};
namespace bh {
int bases_group(const ::bh_bases *b) { return b->group; }   // for the units that see the handle only as an opaque type
}
static inline u32 dense_rec_bytes(int group) { return group == BH_G1 ? 96u : 192u; }
static inline size_t table_bytes(const bh_bases *b) { return b->table ? (size_t)b->tab.W * b->n * b->table_stride : 0; }
// ONE snapshot of a handle's sources for a job, under job_mu (the caller has reserved its job slot: bh_ctx_trim leaves
// tables alone while a call is issuing): the pointers and the strides they are read at come from the same moment - a
// trim + bh_bases_precompute between two reads of the handle could pair a freed table with the other stride
static MsmBases bases_snapshot(bh_ctx *ctx, const bh_bases *b) {
  std::lock_guard<std::mutex> g(ctx->c.job_mu);
  MsmBases s;
  s.dense = {b->dev, dense_rec_bytes(b->group)};
  if (b->padded) s.padded = {b->padded, 128u};
  if (b->table) s.table = {b->table, b->table_stride};
  s.tab = b->tab;
  s.n = b->n;
  return s;
}
// forgets the handle's automatic table in the context's books (caller holds job_mu; the table itself is the caller's to free)
static void forget_auto_table(bh_bases *b) {
  Context &c = b->ctx->c;
  c.tables.erase(std::remove(c.tables.begin(), c.tables.end(), b), c.tables.end());
  const size_t bytes = table_bytes(b);
  c.table_bytes = c.table_bytes > bytes ? c.table_bytes - bytes : 0;
  b->auto_table = false;
}
// a scalar vector resident in HBM (bh_scalars_*): create_proof hands the same assignment to up to four multiexps
struct bh_scalars {
  bh_ctx *ctx;
  void *dev;
  size_t n;
  int fmt;
  bool pooled;   // dev came from the context's pool (else: adopted from the caller, not freed)
};
struct bh_msm_job {
  MsmJobImpl *impl;
};

// hipMalloc'ed block freed on scope exit unless released: the BH_HIP_CHECK early returns of the register /
// read paths must not leak device memory
struct DevGuard {
  void *p = nullptr;
  DevGuard() = default;
  DevGuard(const DevGuard &) = delete;
  DevGuard &operator=(const DevGuard &) = delete;
  ~DevGuard() { if (p) (void)hipFree(p); }
  void *release() { void *q = p; p = nullptr; return q; }
};

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

static inline hipStream_t pick_stream(bh_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->c.stream; }

extern "C" {

const char *bh_version(void) { return "bellman_hip 0.4 (gfx950, built " __DATE__ " " __TIME__ ")"; }

// A proof keeps 6-7 job streams in flight (one per multiexp + the h block); the HIP runtime multiplexes streams onto
// GPU_MAX_HW_QUEUES hardware queues, 4 by default, and jobs that share a queue run one after the other (MiMC-322
// proof 2.99 ms with 4 queues, 2.23 ms with 16; 12 concurrent 2^20 proofs 33.1 -> 36.2 /s:
// profiles/archive/r2_call12_hw_queues.txt).  The runtime reads the variable when it initialises, so the host program calls
// bh_runtime_configure() before its first HIP call (the Python loader and bench.py set the variable themselves); the
// library no longer touches the environment behind the caller's back when it is loaded.
static std::atomic<bool> g_hip_touched{false};      // this library has made a HIP call
static std::atomic<bool> g_configured_early{false};
int bh_runtime_configure(void) {
  const bool early = !g_hip_touched.load();
  setenv("GPU_MAX_HW_QUEUES", "16", 0);   // (no overwrite: a value the caller chose stays)
  if (early) g_configured_early.store(true);
  return early ? 1 : 0;
}

int bh_ctx_create(int device, bh_ctx **out) {
  int count = 0;
  const int queues_env = env_hw_queues();
  const bool early = g_configured_early.load() || (!g_hip_touched.load() && queues_env > 0);
  g_hip_touched.store(true);
  if (hipGetDeviceCount(&count) != hipSuccess || count <= device || device < 0) return BH_ERR_NO_DEVICE;
  BH_HIP_CHECK(hipSetDevice(device));
  bh_ctx *ctx = new bh_ctx();
  ctx->c.device = device;
  ctx->c.hw_queues_env = queues_env;
  ctx->c.configured_early = early;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    ctx->c.num_cus = prop.multiProcessorCount;
    ctx->c.hbm_total = prop.totalGlobalMem;
  }
  // jobs in flight per context: a 2^20-term multiexp holds ~0.6 GB of workspace - by default as many as fit a
  // quarter of the device's memory at that size, at least 8 (create_proof issues 8, prover.rs:244-318)
  {
    long v = env().max_jobs;
    if (v <= 0) v = (long)(ctx->c.hbm_total / 4 / (size_t(640) << 20));
    ctx->c.max_jobs = (uint32_t)(v < 8 ? 8 : v > 4096 ? 4096 : v);
  }
  const EnvSettings &e = env();
  ctx->c.table_budget = e.table_budget != EnvSettings::UNSET ? e.table_budget : ctx->c.hbm_total / 4;
  ctx->c.fft_table_budget = e.fft_table_budget != EnvSettings::UNSET ? e.fft_table_budget : ctx->c.hbm_total / 8;
  if (e.pool_cap != EnvSettings::UNSET) ctx->c.pool.set_cap(e.pool_cap);
  Context *cp = &ctx->c;
  ctx->c.pool.set_pressure_handler([cp] { return msm_complete_oldest(*cp); });
  BH_HIP_CHECK(hipStreamCreateWithFlags(&ctx->c.stream, hipStreamNonBlocking));
  *out = ctx;
  return BH_OK;
}
int bh_ctx_set_limits(bh_ctx *ctx, uint32_t max_jobs_in_flight, size_t pool_cap_bytes, size_t table_budget_bytes,
                      size_t fft_table_budget_bytes) {
  if (!ctx) return BH_ERR_INVALID_ARG;
  if (max_jobs_in_flight) ctx->c.max_jobs = max_jobs_in_flight;
  if (pool_cap_bytes != (size_t)-1) ctx->c.pool.set_cap(pool_cap_bytes);
  if (table_budget_bytes != (size_t)-1) { std::lock_guard<std::mutex> g(ctx->c.job_mu); ctx->c.table_budget = table_budget_bytes; }
  if (fft_table_budget_bytes != (size_t)-1) { std::lock_guard<std::mutex> g(ctx->c.fft_mu); ctx->c.fft_table_budget = fft_table_budget_bytes; }
  return BH_OK;
}
int bh_ctx_info(bh_ctx *ctx, bh_ctx_info_t *info) {
  if (!ctx || !info) return BH_ERR_INVALID_ARG;
  memset(info, 0, sizeof *info);
  info->device = ctx->c.device;
  info->num_cus = (uint32_t)ctx->c.num_cus;
  info->hbm_bytes = ctx->c.hbm_total;
  info->hw_queues_requested = (uint32_t)ctx->c.hw_queues_env;
  info->hw_queues_set_before_hip_init = ctx->c.configured_early ? 1u : 0u;
  info->max_jobs_in_flight = ctx->c.max_jobs;
  info->jobs_in_flight = (uint32_t)msm_jobs_in_flight(ctx->c);
  info->pool_bytes_held = ctx->c.pool.bytes_held();
  info->pool_bytes_idle = ctx->c.pool.bytes_idle();
  {
    std::lock_guard<std::mutex> g(ctx->c.job_mu);
    info->table_bytes = ctx->c.table_bytes;
    info->table_budget = ctx->c.table_budget;
  }
  {
    std::lock_guard<std::mutex> g(ctx->c.fft_mu);
    info->fft_table_bytes = ctx->c.fft_table_bytes;
    info->fft_table_budget = ctx->c.fft_table_budget;
  }
  return BH_OK;
}
int bh_ctx_trim(bh_ctx *ctx) {
  // Workspaces of finished jobs are kept in a size-bucketed cache (a 2^26-term multiexp leaves ~30 GB
  // there): hand the idle blocks and the cached FFT tables back to the driver.  Blocks in use stay.
  if (!ctx) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  BH_HIP_CHECK(hipDeviceSynchronize());
  ctx->c.pool.release_all();
  {
    // window tables built automatically at registration are a cache too (the handles stay usable without them;
    // bh_bases_precompute rebuilds one on request) - unless a multiexp is still in flight: a job issued with BH_MSM_HOLD
    // and not yet started has captured its table pointer but enqueued nothing the device synchronise above could have
    // waited for, so the tables stay until a trim finds the context idle
    std::lock_guard<std::mutex> g(ctx->c.job_mu);
    if (ctx->c.inflight.empty() && ctx->c.issuing == 0) {
      while (!ctx->c.tables.empty()) {
        bh_bases *b = ctx->c.tables.back();
        forget_auto_table(b);
        if (b->table) (void)hipFree(b->table);
        b->table = nullptr;
      }
      ctx->c.table_bytes = 0;   // (as before: the count also covers the tables of prepared verifying keys, pairing.hip)
    }
  }
  {
    std::unique_lock<std::shared_mutex> ex(ctx->c.fft_use_mu);   // no transform between its table lookup and its launches
    BH_HIP_CHECK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> g(ctx->c.fft_mu);
    for (auto &kv : ctx->c.fft_tables) fft_tables_free(kv.second);
    ctx->c.fft_tables.clear();
    ctx->c.fft_table_bytes = 0;
    fft_master_free(ctx->c);
  }
  return BH_OK;
}
void bh_ctx_destroy(bh_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  (void)hipDeviceSynchronize();
  for (auto &kv : ctx->c.fft_tables) fft_tables_free(kv.second);
  fft_master_free(ctx->c);
  ctx->c.pool.release_all();
  {
    // base handles that outlive the context (a host that releases them later - Python objects collected after the
    // Worker was closed) keep their memory, tables included, and must not reach back into the context's bookkeeping
    std::lock_guard<std::mutex> g(ctx->c.job_mu);
    for (bh_bases *b : ctx->c.tables) { b->auto_table = false; b->ctx = nullptr; }
    ctx->c.tables.clear();
    ctx->c.table_bytes = 0;
  }
  for (auto &r : ctx->c.job_pool) {
    for (int i = 0; i < 4; i++) if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
    if (r.dep_event) (void)hipEventDestroy(r.dep_event);
    if (r.acc_event) (void)hipEventDestroy(r.acc_event);
    if (r.sort_event) (void)hipEventDestroy(r.sort_event);
    if (r.pinned) (void)hipHostFree(r.pinned);
    if (r.stream) (void)hipStreamDestroy(r.stream);
  }
  ctx->c.job_pool.clear();
  for (hipStream_t st : ctx->c.stream_pool) (void)hipStreamDestroy(st);
  ctx->c.stream_pool.clear();
  for (hipEvent_t ev : ctx->c.barrier_events) (void)hipEventDestroy(ev);
  ctx->c.barrier_events.clear();
  for (hipStream_t st : ctx->c.hp_streams) (void)hipStreamDestroy(st);
  ctx->c.hp_streams.clear();
  ctx->c.hp_stream_pool.clear();
  if (ctx->c.stream) (void)hipStreamDestroy(ctx->c.stream);
  delete ctx;
}
uint32_t bh_ctx_log_num_cus(const bh_ctx *ctx) {
  uint32_t p = 0;
  while ((1u << (p + 1)) <= (uint32_t)ctx->c.num_cus) p++;
  return p;
}
// served from the context's size-bucketed pool: hipMalloc / hipFree synchronise the device and a
// prover allocates the same handful of vectors for every proof
int bh_dev_alloc(bh_ctx *ctx, size_t bytes, void **dev_ptr) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  *dev_ptr = ctx->c.pool.acquire(bytes);
  return *dev_ptr ? BH_OK : BH_ERR_HIP;
}
int bh_dev_free(bh_ctx *ctx, void *dev_ptr) {
  // callers free after synchronising on the work that used the buffer (bh_msm_wait / bh_ctx_synchronize)
  ctx->c.pool.release(dev_ptr);
  return BH_OK;
}
int bh_dev_upload(bh_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));   // entry points may be called from any host thread
  BH_HIP_CHECK(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->c.stream));
  BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  return BH_OK;
}
int bh_dev_download(bh_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  BH_HIP_CHECK(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->c.stream));
  BH_HIP_CHECK(hipStreamSynchronize(ctx->c.stream));
  return BH_OK;
}
int bh_dev_zero(bh_ctx *ctx, void *dev_ptr, size_t bytes) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (bytes) BH_HIP_CHECK(hipMemsetAsync(dev_ptr, 0, bytes, ctx->c.stream));
  return BH_OK;
}
int bh_stream_create(bh_ctx *ctx, void **stream) {
  // recycled through the context: hipStreamCreate / Destroy cost about a millisecond together, which was a third of
  // a MiMC-sized proof (one stream per proof, groth16_prover.cpp)
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  {
    std::lock_guard<std::mutex> g(ctx->c.job_mu);
    if (!ctx->c.stream_pool.empty()) {
      *stream = (void *)ctx->c.stream_pool.back();
      ctx->c.stream_pool.pop_back();
      return BH_OK;
    }
  }
  hipStream_t st = nullptr;
  BH_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *stream = (void *)st;
  return BH_OK;
}
int bh_stream_create_priority(bh_ctx *ctx, int high, void **stream) {
  if (!high) return bh_stream_create(ctx, stream);
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  {
    std::lock_guard<std::mutex> g(ctx->c.job_mu);
    if (!ctx->c.hp_stream_pool.empty()) {
      *stream = (void *)ctx->c.hp_stream_pool.back();
      ctx->c.hp_stream_pool.pop_back();
      return BH_OK;
    }
  }
  int lo = 0, hi = 0;   // numerically lower = higher priority
  BH_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  hipStream_t st = nullptr;
  BH_HIP_CHECK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
  std::lock_guard<std::mutex> g(ctx->c.job_mu);
  ctx->c.hp_streams.push_back(st);
  *stream = (void *)st;
  return BH_OK;
}
int bh_stream_destroy(bh_ctx *ctx, void *stream) {
  // the caller has synchronised the stream; it goes back to the pool (destroyed with the context)
  if (!stream) return BH_OK;
  std::lock_guard<std::mutex> g(ctx->c.job_mu);
  for (hipStream_t h : ctx->c.hp_streams)
    if (h == (hipStream_t)stream) { ctx->c.hp_stream_pool.push_back(h); return BH_OK; }
  ctx->c.stream_pool.push_back((hipStream_t)stream);
  return BH_OK;
}
int bh_stream_synchronize(bh_ctx *ctx, void *stream) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  BH_HIP_CHECK(hipStreamSynchronize(pick_stream(ctx, stream)));
  return BH_OK;
}
int bh_dev_upload_on(bh_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes, void *stream) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (bytes) BH_HIP_CHECK(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, pick_stream(ctx, stream)));
  return BH_OK;
}
int bh_dev_zero_on(bh_ctx *ctx, void *dev_ptr, size_t bytes, void *stream) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  if (bytes) BH_HIP_CHECK(hipMemsetAsync(dev_ptr, 0, bytes, pick_stream(ctx, stream)));
  return BH_OK;
}
int bh_ctx_accumulations_after(bh_ctx *ctx, void *stream) {
  // the next chip-filling bucket accumulation issued on this context - and through the accumulation chain
  // (common.hpp) every later one - starts after everything enqueued on `stream` so far
  if (!ctx || !stream) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  std::lock_guard<std::mutex> g(ctx->c.acc_mu);
  constexpr size_t RING = 64;   // an event is only referenced until the next accumulation is issued
  if (ctx->c.barrier_events.size() < RING) {
    hipEvent_t ev = nullptr;
    BH_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ctx->c.barrier_events.push_back(ev);
    ctx->c.barrier_next = ctx->c.barrier_events.size() - 1;
  } else {
    ctx->c.barrier_next = (ctx->c.barrier_next + 1) % RING;
  }
  hipEvent_t ev = ctx->c.barrier_events[ctx->c.barrier_next];
  BH_HIP_CHECK(hipEventRecord(ev, (hipStream_t)stream));
  if (ctx->c.pending_barriers.size() < RING / 2) ctx->c.pending_barriers.push_back(ev);
  return BH_OK;
}
int bh_ctx_synchronize(bh_ctx *ctx) {
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  BH_HIP_CHECK(hipDeviceSynchronize());
  return BH_OK;
}

// ---- EvaluationDomain ------------------------------------------------------------------------
int bh_fft_fr_dev(bh_ctx *ctx, void *data_dev, uint32_t log_n, int mode, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = nullptr;
  if (log_n > 11) {   // more than one pass (fft.hip NTT_MAX_R)
    scratch = ctx->c.pool.acquire(sizeof(fr_t) << log_n);
    if (!scratch) return BH_ERR_HIP;
  }
  int rc = ntt_run(ctx->c, (fr_t *)data_dev, (fr_t *)scratch, log_n, mode, st);
  if (scratch) {
    // the scratch buffer may be recycled by another stream: fence before returning it
    if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
    ctx->c.pool.release(scratch);
  }
  return rc;
}
int bh_fft_fr(bh_ctx *ctx, void *data_host, uint32_t log_n, int mode) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  const size_t bytes = sizeof(fr_t) << log_n;
  void *d = ctx->c.pool.acquire(bytes);
  if (!d) return BH_ERR_HIP;
  int rc = bh_dev_upload(ctx, d, data_host, bytes);
  if (rc == BH_OK) rc = bh_fft_fr_dev(ctx, d, log_n, mode, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, data_host, d, bytes);
  ctx->c.pool.release(d);
  return rc;
}
// ---- k vectors per call (fft.hip ntt_run_many) ------------------------------------------------------------------
// Where the batched launches replace k single-vector transforms without being asked to (BH_FFT_MANY_FORCE).  Set from
// profiles/fft_many_bench.json (tools/bench_fft_many.py): a shape is taken only where the batched call's min-of-5 wall time
// is below the baseline's by more than the baseline's own spread in that run.  Shapes nobody measured take the single path.
// Measured (MI355X, 2^6 ... 2^22 points in steps of 4x, k = 2, 4, 16, 64 with k * n <= 2^24; ifft at every k, the four modes
// at k = 4, the h block at every k):
//   transforms  win at every measured shape from 2^6 to 2^20 (2^8 x 64: 0.050 ms against 1.68; 2^16 x 4: 0.069 against
//               0.25; 2^20 x 16: 1.65 against 2.16) and not at 2^22 (0.97 - 1.01 x; one shape of five, coset_fft x 4, is 1 %
//               beyond the spread in one run of two: the passes fill the chip by themselves, and the table entries a
//               group of vectors could share are not what bounds them);
//   h blocks    win from 2^12 to 2^20 at every k (2^14 x 4: 0.36 ms against 1.37), from 2^6 to 2^10 at k >= 4 only (at k = 2
//               the single h block's own three-vector launches are 0.16 - 0.22 ms against 0.22 - 0.34), and not at 2^22
//               (0.91 - 0.96 x).
// The rule covers the measured box and what lies between its points (odd log_n, k = 3, 5 ... 63).  Outside it - fewer than
// 2^6 or more than 2^20 points, k = 1, k > 64, more than 2^24 elements in all - the call issues single-vector transforms.
constexpr uint32_t FFT_MANY_RULE_LOG_N_MIN = 6, FFT_MANY_RULE_LOG_N_MAX = 20, FFT_MANY_RULE_LOG_ELEMS_MAX = 24;
constexpr size_t FFT_MANY_RULE_K_MIN = 2, FFT_MANY_RULE_K_MAX = 64, FFT_MANY_RULE_H_SMALL_K_MIN = 4;
static bool fft_many_wins(uint32_t log_n, size_t k, bool h_block = false) {
  if (log_n < FFT_MANY_RULE_LOG_N_MIN || log_n > FFT_MANY_RULE_LOG_N_MAX || k < FFT_MANY_RULE_K_MIN || k > FFT_MANY_RULE_K_MAX) return false;
  if ((k << log_n) > ((size_t)1 << FFT_MANY_RULE_LOG_ELEMS_MAX)) return false;
  if (h_block && log_n <= 11 && k < FFT_MANY_RULE_H_SMALL_K_MIN) return false;
  return true;
}
// the checks the four calls share; *use_many: batched launches or k single-vector transforms
static int fft_many_args(bh_ctx *ctx, const void *data, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                         bool *use_many, bool h_block = false) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !data || mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  if (stride_bytes < ((size_t)sizeof(fr_t) << log_n) || stride_bytes % sizeof(fr_t)) return BH_ERR_INVALID_ARG;
  if ((flags & ~(unsigned)(BH_FFT_MANY_FORCE | BH_FFT_MANY_SINGLE)) || flags == (BH_FFT_MANY_FORCE | BH_FFT_MANY_SINGLE))
    return BH_ERR_INVALID_ARG;
  *use_many = (flags & BH_FFT_MANY_FORCE) || (!(flags & BH_FFT_MANY_SINGLE) && fft_many_wins(log_n, k, h_block));
  return BH_OK;
}
static bool fft_many_scratch_ok(uint32_t log_n, const void *scratch, size_t scratch_bytes) {
  return log_n <= 11 || (scratch && scratch_bytes >= ((size_t)sizeof(fr_t) << log_n));
}
int bh_fft_fr_many_dev_on(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                          void *scratch_dev, size_t scratch_bytes, void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, data_dev, stride_bytes, k, log_n, mode, flags, &use_many);
  if (rc) return rc;
  if (!fft_many_scratch_ok(log_n, scratch_dev, scratch_bytes)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  const u64 stride = stride_bytes / sizeof(fr_t);
  if (!use_many) return ntt_run_each(ctx->c, (fr_t *)data_dev, stride, k, log_n, mode, (fr_t *)scratch_dev, st);
  return ntt_run_many(ctx->c, (fr_t *)data_dev, stride, k, log_n, mode, (fr_t *)scratch_dev, scratch_bytes >> (log_n + 5), st);
}
int bh_fft_fr_many_dev(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                       void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, data_dev, stride_bytes, k, log_n, mode, flags, &use_many);
  if (rc || !k) return rc;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  if (log_n > 11) {
    // a scratch vector per transformed vector, up to 256 MiB; one vector where the pool cannot give more
    const size_t one = sizeof(fr_t) << log_n;
    size_t vecs = use_many ? k : 1;
    while (vecs > 1 && vecs * one > ((size_t)256 << 20)) vecs = (vecs + 1) / 2;
    scratch = ctx->c.pool.acquire(vecs * one);
    if (!scratch && vecs > 1) { vecs = 1; scratch = ctx->c.pool.acquire(one); }
    if (!scratch) return BH_ERR_HIP;
    scratch_bytes = vecs * one;
  }
  rc = bh_fft_fr_many_dev_on(ctx, data_dev, stride_bytes, k, log_n, mode, flags, scratch, scratch_bytes, stream);
  if (scratch) {
    // the scratch buffer may be recycled by another stream: fence before returning it
    if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
    ctx->c.pool.release(scratch);
  }
  return rc;
}
int bh_fft_fr_many(bh_ctx *ctx, void *data_host, size_t k, uint32_t log_n, int mode) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !data_host || mode < 0 || mode > 3) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  const size_t one = sizeof(fr_t) << log_n, bytes = one * k;
  void *d = ctx->c.pool.acquire(bytes);
  if (!d) return BH_ERR_HIP;
  int rc = bh_dev_upload(ctx, d, data_host, bytes);
  if (rc == BH_OK) rc = bh_fft_fr_many_dev(ctx, d, one, k, log_n, mode, 0, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, data_host, d, bytes);
  ctx->c.pool.release(d);
  return rc;
}
int bh_h_poly_fr_many_dev_on(bh_ctx *ctx, void *a, void *b, void *c, size_t stride_bytes, size_t k, uint32_t log_n, unsigned flags,
                             void *scratch_dev, size_t scratch_bytes, void *stream) {
  bool use_many = false;
  int rc = fft_many_args(ctx, a, stride_bytes, k, log_n, BH_FFT, flags, &use_many, true);
  if (rc) return rc;
  if (!b || !c || !fft_many_scratch_ok(log_n, scratch_dev, scratch_bytes)) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  const u64 stride = stride_bytes / sizeof(fr_t);
  if (!use_many) return h_poly_each_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, stride, k, log_n, (fr_t *)scratch_dev, st);
  return h_poly_many_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, stride, k, log_n, (fr_t *)scratch_dev, scratch_bytes >> (log_n + 5), st);
}
int bh_fr_mul_assign_dev(bh_ctx *ctx, void *a, const void *b, size_t n, void *stream) {
  return fr_mul_assign(ctx->c, (fr_t *)a, (const fr_t *)b, n, pick_stream(ctx, stream));
}
int bh_fr_sub_assign_dev(bh_ctx *ctx, void *a, const void *b, size_t n, void *stream) {
  return fr_sub_assign(ctx->c, (fr_t *)a, (const fr_t *)b, n, pick_stream(ctx, stream));
}
int bh_fr_divide_by_z_on_coset_dev(bh_ctx *ctx, void *a, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  return fr_divide_by_z(ctx->c, (fr_t *)a, log_n, pick_stream(ctx, stream));
}
int bh_fr_distribute_powers_dev(bh_ctx *ctx, void *a, size_t n, const void *g_host, void *stream) {
  fr_t g;
  memcpy(&g, g_host, sizeof g);
  return fr_distribute_powers(ctx->c, (fr_t *)a, n, g, pick_stream(ctx, stream));
}
// ---- EvaluationDomain<Fr, Point<G>> (point_fft.hip) ----------------------------------------------
static bool group_ok(int group) { return group == BH_G1 || group == BH_G2; }
int bh_fft_point_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, int mode, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !group_ok(group) || mode < 0 || mode > 3 || !points_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_fft(ctx->c, group, points_dev, log_n, mode, pick_stream(ctx, stream));
}
int bh_point_distribute_powers_dev(bh_ctx *ctx, int group, void *points_dev, size_t n, const void *g_host, void *stream) {
  if (!ctx || !group_ok(group) || !g_host) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  fr_t g;
  memcpy(&g, g_host, sizeof g);
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_distribute_powers(ctx->c, group, points_dev, n, g, pick_stream(ctx, stream));
}
int bh_point_divide_by_z_on_coset_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !group_ok(group) || !points_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_divide_by_z(group, points_dev, log_n, pick_stream(ctx, stream));
}
int bh_point_mul_assign_dev(bh_ctx *ctx, int group, void *points_dev, const void *scalars_dev, size_t n, void *stream) {
  if (!ctx || !group_ok(group)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_mul_assign(group, points_dev, scalars_dev, n, pick_stream(ctx, stream));
}
int bh_point_sub_assign_dev(bh_ctx *ctx, int group, void *a_dev, const void *b_dev, size_t n, void *stream) {
  if (!ctx || !group_ok(group)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return point_sub_assign(group, a_dev, b_dev, n, pick_stream(ctx, stream));
}
int bh_fr_powers_dev(bh_ctx *ctx, void *out, size_t n, const void *g_host, const void *scale_host, void *stream) {
  fr_t g, sc;
  memcpy(&g, g_host, sizeof g);
  memcpy(&sc, scale_host, sizeof sc);
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return fr_gen_powers(ctx->c, (fr_t *)out, n, g, sc, pick_stream(ctx, stream));
}
int bh_h_poly_fr_dev_on(bh_ctx *ctx, void *a, void *b, void *c, void *scratch, uint32_t log_n, void *stream) {
  // enqueue only: the caller owns `scratch` (2^log_n Fr; may be null up to 2^11) until the stream has drained
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  if (!ctx || !a || !b || !c || (log_n > 11 && !scratch)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return h_poly_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, (fr_t *)scratch, log_n, pick_stream(ctx, stream));
}
int bh_h_poly_fr_dev(bh_ctx *ctx, void *a, void *b, void *c, uint32_t log_n, void *stream) {
  if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  void *scratch = ctx->c.pool.acquire(sizeof(fr_t) << log_n);
  if (!scratch) return BH_ERR_HIP;
  int rc = h_poly_dev(ctx->c, (fr_t *)a, (fr_t *)b, (fr_t *)c, (fr_t *)scratch, log_n, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  ctx->c.pool.release(scratch);
  return rc;
}
int bh_h_poly_fr(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host, size_t n_evals,
                 void *h_out_host, size_t *h_len) {
  // EvaluationDomain::from_coeffs (domain.rs:47-79): m = next power of two >= len, zero padded
  uint32_t log_n = 0;
  size_t m = 1;
  while (m < n_evals) {
    m *= 2;
    log_n++;
    if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  }
  const size_t bytes = sizeof(fr_t) * m, in_bytes = sizeof(fr_t) * n_evals;
  void *d[3] = {ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes)};
  const void *h[3] = {a_host, b_host, c_host};
  int rc = (d[0] && d[1] && d[2]) ? BH_OK : BH_ERR_HIP;
  for (int i = 0; i < 3 && rc == BH_OK; i++) {
    if (hipMemsetAsync(d[i], 0, bytes, ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;
    if (rc == BH_OK && in_bytes &&
        hipMemcpyAsync(d[i], h[i], in_bytes, hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess)
      rc = BH_ERR_HIP;
  }
  if (rc == BH_OK) rc = bh_h_poly_fr_dev(ctx, d[0], d[1], d[2], log_n, nullptr);
  if (rc == BH_OK) rc = bh_dev_download(ctx, h_out_host, d[0], sizeof(fr_t) * (m - 1));   // prover.rs:238-239
  if (h_len) *h_len = m - 1;
  for (int i = 0; i < 3; i++) ctx->c.pool.release(d[i]);
  return rc;
}

int bh_h_poly_fr_scalars(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host, size_t n_evals,
                         bh_scalars **h_out) {
  if (!ctx || !h_out || (n_evals && (!a_host || !b_host || !c_host))) return BH_ERR_INVALID_ARG;
  uint32_t log_n = 0;
  size_t m = 1;
  while (m < n_evals) {   // EvaluationDomain::from_coeffs (domain.rs:47-79)
    m *= 2;
    log_n++;
    if (log_n >= 32) return BH_ERR_DEGREE_TOO_LARGE;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t bytes = sizeof(fr_t) * m, in_bytes = sizeof(fr_t) * n_evals;
  // the three vectors are staged on three streams so that the copies of b and c overlap the first transforms... the
  // h block itself is a dependent chain, so: one caller-private stream (concurrent proofs do not serialise on the
  // context stream)
  void *stv = nullptr;
  int rc = bh_stream_create(ctx, &stv);
  if (rc != BH_OK) return rc;
  hipStream_t st = (hipStream_t)stv;
  void *d[3] = {ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes), ctx->c.pool.acquire(bytes)};
  void *scratch = log_n > 11 ? ctx->c.pool.acquire(bytes) : nullptr;
  const void *h[3] = {a_host, b_host, c_host};
  rc = (d[0] && d[1] && d[2] && (log_n <= 11 || scratch)) ? BH_OK : BH_ERR_HIP;
  for (int i = 0; i < 3 && rc == BH_OK; i++) {
    if (m > n_evals && hipMemsetAsync((char *)d[i] + in_bytes, 0, bytes - in_bytes, st) != hipSuccess) rc = BH_ERR_HIP;
    if (rc == BH_OK && in_bytes && hipMemcpyAsync(d[i], h[i], in_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
      rc = BH_ERR_HIP;
  }
  if (rc == BH_OK) rc = h_poly_dev(ctx->c, (fr_t *)d[0], (fr_t *)d[1], (fr_t *)d[2], (fr_t *)scratch, log_n, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  (void)bh_stream_destroy(ctx, stv);
  ctx->c.pool.release(d[1]);
  ctx->c.pool.release(d[2]);
  ctx->c.pool.release(scratch);
  if (rc != BH_OK) { ctx->c.pool.release(d[0]); return rc; }
  *h_out = new bh_scalars{ctx, d[0], m - 1, BH_SCALARS_MONT, true};   // a.len() - 1 coefficients, prover.rs:238-239
  return BH_OK;
}

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

// ---- multiexp -----------------------------------------------------------------------------------
// multiexp of a handful of terms on the host, at issue time (src/multiexp.rs:210-332 semantics incl. the error
// precedence of Appendix A item 6).  Returns false when the case is not eligible (bases beyond the mirrored prefix).
static bool tiny_msm_on_host(const bh_bases *bases, size_t skip, const void *scalars_host, size_t n, int fmt,
                             const uint64_t *density_host, int *rc_out, unsigned char *result) {
  const size_t rec = bases->group == BH_G1 ? 96 : 192;
  const size_t have = bases->host_prefix.size() / rec;
  if (bases->n > have && skip + n > have) return false;   // a base index could fall outside the mirror
  memset(result, 0, rec);
  // pass 1: base index of every dense entry, error conditions
  fr_t sc[TINY_MSM_MAX];
  size_t base_of[TINY_MSM_MAX];
  bool dense[TINY_MSM_MAX];
  size_t cursor = skip;
  bool eof = false, ident = false, ident_top = false;
  // the reference's window size for fewer than 32 terms is 3 (multiexp.rs:318-319): top window = bits [252, 255)
  const u32 lo_ref = 3 * ((255 + 2) / 3 - 1);
  for (size_t i = 0; i < n; i++) {
    dense[i] = density_host ? ((density_host[i >> 6] >> (i & 63)) & 1) : true;
    if (!dense[i]) continue;
    base_of[i] = cursor++;
    memcpy(&sc[i], (const char *)scalars_host + i * 32, 32);
    if (fmt == BH_SCALARS_MONT) {
      fe_from_mont(sc[i], sc[i]);
    } else {
      for (int k = 0; k < 2; k++) {   // values in [q, 2^256) are taken mod q, as on the device
        fr_t t;
        u32 br = 0;
        for (int w = 0; w < 8; w++) t.l[w] = subb(sc[i].l[w], FrParams::mod(w), br, br);
        if (!br) sc[i] = t;
      }
    }
    if (base_of[i] >= bases->n) { eof = true; dense[i] = false; continue; }   // every dense entry checks EOF first
    if (fe_is_zero(sc[i])) continue;                                          // a zero scalar skips its base unseen
    const unsigned char *b = bases->host_prefix.data() + base_of[i] * rec;
    bool is_id = true;
    for (size_t k = 0; k < rec; k++) is_id &= b[k] == 0;
    if (is_id) {
      ident = true;
      bool top = false;
      for (u32 bit = lo_ref; bit < 256; bit++) top |= (sc[i].l[bit >> 5] >> (bit & 31)) & 1;
      if (top && !eof) ident_top = true;   // in the top window, before the first EOF entry
    }
  }
  if (eof && ident) { *rc_out = ident_top ? BH_ERR_UNEXPECTED_IDENTITY : BH_ERR_UNEXPECTED_EOF; return true; }
  if (eof) { *rc_out = BH_ERR_UNEXPECTED_EOF; return true; }
  if (ident) { *rc_out = BH_ERR_UNEXPECTED_IDENTITY; return true; }
  // pass 2: the sum
  alignas(16) unsigned char acc[192], term[192];
  memset(acc, 0, sizeof acc);
  fr_t one;
  fe_zero(one);
  one.l[0] = 1;
  for (size_t i = 0; i < n; i++) {
    if (!dense[i] || fe_is_zero(sc[i])) continue;
    const unsigned char *b = bases->host_prefix.data() + base_of[i] * rec;
    if (fe_eq(sc[i], one)) memcpy(term, b, rec); else host_point_mul(bases->group, term, b, &sc[i]);
    host_point_add(bases->group, acc, acc, term, 1);
  }
  memcpy(result, acc, rec);
  *rc_out = BH_OK;
  return true;
}

static int msm_common(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars, bool scalars_on_host,
                      size_t n, int fmt, const uint64_t *density, bool density_on_host, size_t density_len,
                      const bh_msm_opts *o, bh_msm_job **out, u64 shard_ref_n = 0, void *after_stream = nullptr,
                      u32 many_vectors = 0, u64 many_stride = 0) {
  if (!ctx || !bases || !out) return BH_ERR_INVALID_ARG;
  MsmOpts opts;
  opts.vectors = many_vectors; opts.scalar_stride = many_stride;   // (a many-job: resident scalars only, bh_msm_many_*)
  if (shard_ref_n) { opts.ref_n = shard_ref_n; opts.always_resolve_ident = true; }
  if (o) {
    if (o->window_bits && (o->window_bits < 2 || o->window_bits > 24)) return BH_ERR_INVALID_ARG;
    opts.c = o->window_bits; opts.chunk = o->chunk; opts.flags = o->flags;
  }
  if (fmt != BH_SCALARS_CANONICAL && fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  if (density && density_len != n) return BH_ERR_INVALID_ARG;   // multiexp.rs:324-329 (assert)
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  // back-pressure (src/multicore.rs:47-73): at the cap the issuing thread completes the oldest job itself
  while (!msm_slot_try_reserve(ctx->c))
    if (!msm_complete_oldest(ctx->c)) std::this_thread::yield();   // the slots are held by calls still issuing
  const MsmBases src = bases_snapshot(ctx, bases);   // (after the slot is reserved)
  MsmJobImpl *impl = msm_job_new(&ctx->c, bases->group);
  if (!impl) { msm_slot_release(ctx->c); return BH_ERR_HIP; }
  if (n && n <= TINY_MSM_MAX && scalars_on_host && (!density || density_on_host) && !(opts.flags & BH_MSM_NO_SMALL_PATH) &&
      !shard_ref_n) {
    int trc = BH_OK;
    alignas(16) unsigned char res[192];
    if (tiny_msm_on_host(bases, skip, scalars, n, fmt, density, &trc, res)) {
      msm_job_set_result(*impl, trc, trc == BH_OK ? res : nullptr);
      msm_job_track(*impl);   // trivial: only gives the slot back
      *out = new bh_msm_job{impl};
      return BH_OK;
    }
  }
  hipStream_t st = msm_job_stream(*impl);
  const void *sc_dev = scalars;
  const u64 *dn_dev = density;
  int rc = BH_OK;
  if (after_stream) rc = msm_job_after(*impl, (hipStream_t)after_stream);
  if (rc == BH_OK && n && scalars_on_host) {
    void *p = ctx->c.pool.acquire(n * 32);
    if (!p) rc = BH_ERR_HIP;
    else {
      msm_job_own(*impl, p);
      if (hipMemcpyAsync(p, scalars, n * 32, hipMemcpyHostToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
      sc_dev = p;
    }
  }
  if (rc == BH_OK && n && density && density_on_host) {
    const size_t nw = (n + 63) / 64;
    void *p = ctx->c.pool.acquire(nw * 8);
    if (!p) rc = BH_ERR_HIP;
    else {
      msm_job_own(*impl, p);
      if (hipMemcpyAsync(p, density, nw * 8, hipMemcpyHostToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
      dn_dev = (const u64 *)p;
    }
  }
  if (rc == BH_OK) rc = msm_job_enqueue(*impl, src, skip, sc_dev, n, fmt, dn_dev, opts);
  if (rc != BH_OK) {
    float ms[4];
    unsigned char dummy[192];
    (void)msm_job_finish(*impl, dummy, ms);
    msm_job_delete(impl);
    msm_slot_release(ctx->c);
    return rc;
  }
  msm_job_track(*impl);
  *out = new bh_msm_job{impl};
  return BH_OK;
}
// ---- several scalar vectors over one base vector in ONE job ---------------------------------------
struct bh_msm_many_job {
  bh_ctx *ctx = nullptr;
  const bh_bases *bases = nullptr;
  size_t skip = 0, stride = 0, n = 0, k = 0, dlen = 0;
  int fmt = 0;
  const void *sc_dev = nullptr;       // resident scalars (the caller's, or this job's upload)
  const u64 *dn_dev = nullptr;
  bh_msm_opts o = {0, 0, 0};          // for the ordinary jobs: without BH_MSM_MANY_FORCE
  std::vector<void *> owned;          // uploads of the host entry, kept until the wait (the error path reads them again)
  bh_msm_job *many = nullptr;         // the many-plan job, or
  std::vector<bh_msm_job *> singles;  // k ordinary jobs issued together
};
// Where the many-plan replaces k ordinary jobs without being asked to (BH_MSM_MANY_FORCE).  Set from
// profiles/msm_many_bench.json (tools/bench_msm_many.py): the many-plan is chosen only at shapes where its min-of-5 wall
// time is below the baseline's by more than the baseline's own spread in that run.
// Measured (MI355X, G1 2^10 ... 2^20 and G2 2^10 ... 2^18 terms in steps of 4x, k = 2, 4, 8, 16, bases with their
// automatic window table): the table flavour wins at every measured shape with 4 <= k <= 16 and 2^10 <= n <= 2^18 in both
// groups (G1 2^12 x 16: 1.02 ms against 2.73; 2^16 x 8: 2.52 against 3.41; G2 2^18 x 16: 35.9 against 47.8); at k = 2 it wins
// at six shapes of eleven in that run and at three in the run before, and at 2^20 (20-bit rows, 2^19 buckets per vector) nowhere.  The rule covers the measured
// box and what lies between its points (k = 5 ... 15, the odd powers of two).  Outside it the call issues ordinary jobs:
// the classic flavour, fewer than 2^10 or more than 2^18 terms, k < 4, and k > 16 - not measured, and the job's workspace
// grows with k.
constexpr size_t MANY_RULE_K_MIN = 4, MANY_RULE_K_MAX = 16, MANY_RULE_LOG_N_MIN = 10, MANY_RULE_LOG_N_MAX = 18;
static bool many_plan_wins(int group, size_t n, size_t k, bool table) {
  (void)group;
  return table && k >= MANY_RULE_K_MIN && k <= MANY_RULE_K_MAX && n >= ((size_t)1 << MANY_RULE_LOG_N_MIN) &&
         n <= ((size_t)1 << MANY_RULE_LOG_N_MAX);
}
static void many_job_free(bh_msm_many_job *mj) {
  for (void *p : mj->owned) mj->ctx->c.pool.release(p);
  delete mj;
}
static int many_issue_singles(bh_msm_many_job *mj, void *after_stream) {
  for (size_t v = 0; v < mj->k; v++) {
    bh_msm_job *j = nullptr;
    const int rc = msm_common(mj->ctx, mj->bases, mj->skip, (const char *)mj->sc_dev + v * mj->stride, false, mj->n, mj->fmt,
                              mj->dn_dev, false, mj->dlen, &mj->o, &j, 0, after_stream);
    if (rc != BH_OK) {
      unsigned char sink[192];
      for (bh_msm_job *q : mj->singles) (void)bh_msm_wait(q, sink);
      mj->singles.clear();
      return rc;
    }
    mj->singles.push_back(j);
  }
  return BH_OK;
}
static int many_common(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars, bool on_host, size_t stride,
                       size_t n, size_t k, int fmt, const uint64_t *density, size_t density_len, const bh_msm_opts *opts,
                       void *after_stream, bh_msm_many_job **out) {
  if (!ctx || !bases || !out || (k && n && !scalars)) return BH_ERR_INVALID_ARG;
  if (fmt != BH_SCALARS_CANONICAL && fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  if (k && (stride % 32 || stride / 32 < n)) return BH_ERR_INVALID_ARG;
  if (density && density_len != n) return BH_ERR_INVALID_ARG;   // multiexp.rs:324-329 (assert)
  if (opts && (opts->flags & BH_MSM_HOLD)) return BH_ERR_INVALID_ARG;
  if (opts && opts->window_bits && (opts->window_bits < 2 || opts->window_bits > 24)) return BH_ERR_INVALID_ARG;
  std::unique_ptr<bh_msm_many_job> mj(new bh_msm_many_job());
  mj->ctx = ctx; mj->bases = bases; mj->skip = skip; mj->stride = stride; mj->n = n; mj->k = k; mj->fmt = fmt;
  mj->dlen = density ? density_len : 0;
  if (opts) mj->o = *opts;
  const bool force = (mj->o.flags & BH_MSM_MANY_FORCE) != 0;
  mj->o.flags &= ~BH_MSM_MANY_FORCE;
  if (k == 0) { *out = mj.release(); return BH_OK; }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  auto fail = [&](int rc) { many_job_free(mj.release()); return rc; };
  if (on_host && n && n <= TINY_MSM_MAX) {
    // a handful of terms: every vector is answered as the single call answers it (on the host, at issue time)
    for (size_t v = 0; v < k; v++) {
      bh_msm_job *j = nullptr;
      const int rc = msm_common(ctx, bases, skip, (const char *)scalars + v * stride, true, n, fmt, density, true, mj->dlen,
                                &mj->o, &j);
      if (rc != BH_OK) {
        unsigned char sink[192];
        for (bh_msm_job *q : mj->singles) (void)bh_msm_wait(q, sink);
        return fail(rc);
      }
      mj->singles.push_back(j);
    }
    *out = mj.release();
    return BH_OK;
  }
  mj->sc_dev = scalars; mj->dn_dev = density;
  if (on_host && n) {
    // one upload each for the k vectors and the density map, on the context's stream: resident before any job reads them,
    // and until the wait (the error path answers every vector from them again)
    const size_t bytes = (k - 1) * stride + n * 32;
    void *p = ctx->c.pool.acquire(bytes);
    if (!p) return fail(BH_ERR_HIP);
    mj->owned.push_back(p);
    if (hipMemcpyAsync(p, scalars, bytes, hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess) return fail(BH_ERR_HIP);
    mj->sc_dev = p;
    if (density) {
      const size_t nw = (n + 63) / 64;
      void *d = ctx->c.pool.acquire(nw * 8);
      if (!d) return fail(BH_ERR_HIP);
      mj->owned.push_back(d);
      if (hipMemcpyAsync(d, density, nw * 8, hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess) return fail(BH_ERR_HIP);
      mj->dn_dev = (const u64 *)d;
    }
    if (hipStreamSynchronize(ctx->c.stream) != hipSuccess) return fail(BH_ERR_HIP);
  }
  bool use_many = k > 1 && n > 0;
  if (use_many && !force) {
    MsmOpts mo;
    mo.c = mj->o.window_bits; mo.flags = mj->o.flags;
    // (the plan the job would run; the accumulate form, chosen in msm_enqueue, has no part in that)
    use_many = many_plan_wins(bases->group, n, k, msm_pick_sources(bases_snapshot(ctx, bases), mo, n, bases->group, ACC_MULTI_LANE).use_table);
  }
  int rc;
  if (use_many) {
    rc = msm_common(ctx, bases, skip, mj->sc_dev, false, n, fmt, mj->dn_dev, false, mj->dlen, &mj->o, &mj->many, 0, after_stream,
                    (u32)std::min<size_t>(k, 0xffffffffu), stride);
    // chosen by the rule, not forced: a plan the pipeline cannot index, or a workspace the pool cannot give, is no error of
    // the caller's - the ordinary jobs serve the call (the failed job has released what it held)
    if (rc != BH_OK && !force) rc = many_issue_singles(mj.get(), after_stream);
  } else {
    rc = many_issue_singles(mj.get(), after_stream);
  }
  if (rc != BH_OK) return fail(rc);
  *out = mj.release();
  return BH_OK;
}
int bh_msm_many_async_dev(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t stride_bytes,
                          size_t n_scalars, size_t k, int scalar_fmt, const uint64_t *density_words_dev, size_t density_len,
                          const bh_msm_opts *opts, void *after_stream, bh_msm_many_job **job) {
  return many_common(ctx, bases, skip, scalars_dev, false, stride_bytes, n_scalars, k, scalar_fmt, density_words_dev, density_len,
                     opts, after_stream, job);
}
int bh_msm_many_async(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host, size_t stride_bytes,
                      size_t n_scalars, size_t k, int scalar_fmt, const uint64_t *density_words, size_t density_len,
                      const bh_msm_opts *opts, bh_msm_many_job **job) {
  return many_common(ctx, bases, skip, scalars_host, true, stride_bytes, n_scalars, k, scalar_fmt, density_words, density_len, opts,
                     nullptr, job);
}
int bh_msm_many_wait(bh_msm_many_job *job, void *out_affine_k, int32_t *rcs_k, float *stage_ms4, uint64_t *stats8) {
  if (!job) return BH_ERR_INVALID_ARG;
  std::unique_ptr<bh_msm_many_job, void (*)(bh_msm_many_job *)> mj(job, many_job_free);
  const size_t rec = mj->bases ? (mj->bases->group == BH_G1 ? 96 : 192) : 0;
  float ms[4] = {0, 0, 0, 0};
  u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int call_rc = BH_OK;
  if (mj->k && (!out_affine_k || !rcs_k)) call_rc = BH_ERR_INVALID_ARG;   // (the jobs are still waited on and freed)
  std::vector<unsigned char> scratch(mj->k * rec + 192);
  unsigned char *out = call_rc == BH_OK && out_affine_k ? (unsigned char *)out_affine_k : scratch.data();
  std::vector<int32_t> rcs(mj->k, BH_OK);
  if (mj->many) {
    bool fallback = false;
    MsmJobImpl *impl = mj->many->impl;
    int rc = msm_job_finish_many(*impl, out, mj->k, ms, st, &fallback);
    msm_job_delete(impl);
    delete mj->many;
    mj->many = nullptr;
    if (rc < 0) call_rc = rc;
    else if (fallback) {
      // a device flag was set: every vector by the single-vector path, over the inputs that are still resident
      rc = many_issue_singles(mj.get(), nullptr);
      if (rc != BH_OK) call_rc = rc;
    }
  }
  for (size_t v = 0; v < mj->singles.size(); v++) {
    float m1[4];
    u64 s1[8];
    const int rc = bh_msm_wait_stats(mj->singles[v], out + v * rec, m1, s1);
    if (rc < 0) { call_rc = rc; continue; }
    rcs[v] = rc;
    if (rc != BH_OK) memset(out + v * rec, 0, rec);
    for (int q = 0; q < 4; q++) ms[q] += m1[q];
    for (int q = 0; q < 4; q++) st[q] += s1[q];
    for (int q = 4; q < 8; q++) st[q] = s1[q];
  }
  mj->singles.clear();
  if (call_rc == BH_OK && rcs_k) memcpy(rcs_k, rcs.data(), mj->k * sizeof(int32_t));
  if (stage_ms4) memcpy(stage_ms4, ms, sizeof ms);
  if (stats8) memcpy(stats8, st, sizeof st);
  return call_rc;
}
int bh_msm_many_plan_info(size_t n, size_t k, int group, unsigned table_bits, unsigned num_cus, unsigned *out12) {
  if (!out12 || (group != BH_G1 && group != BH_G2) || !k || k >= 65536 || n >= ((size_t)1 << 32)) return BH_ERR_INVALID_ARG;
  if (table_bits && (table_bits < 2 || table_bits > 24)) return BH_ERR_INVALID_ARG;
  const bool g2 = group == BH_G2;
  WindowTable t = {table_bits, table_bits ? (256 + table_bits - 1) / table_bits : 0, n};
  const MsmPlan p = make_many_plan(n, k, table_bits ? &t : nullptr, 0, 0, g2, num_cus ? (int)num_cus : 256);
  if (!many_plan_valid(p, n)) return BH_ERR_INVALID_ARG;
  const u64 W = (u64)p.windows_per_vector * k;
  out12[0] = p.c; out12[1] = (unsigned)W; out12[2] = p.nb; out12[3] = p.chunk; out12[4] = p.chunks_per_window;
  out12[5] = p.sort_passes; out12[6] = p.n; out12[7] = p.vectors; out12[8] = p.windows_per_vector; out12[9] = p.Wd;
  const u64 bytes = job_result_bytes(p, g2 ? 384 : 192);   // what msm_enqueue copies to the job's pinned buffer
  out12[10] = (unsigned)bytes; out12[11] = (unsigned)(bytes >> 32);
  return BH_OK;
}
// ---- scalars resident in HBM --------------------------------------------------------------------
int bh_scalars_register(bh_ctx *ctx, const void *scalars_host, size_t n, int scalar_fmt, bh_scalars **out) {
  if (!ctx || !out || (n && !scalars_host)) return BH_ERR_INVALID_ARG;
  if (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  void *d = ctx->c.pool.acquire(n ? n * 32 : 32);
  if (!d) return BH_ERR_HIP;
  if (n) {
    // pageable host memory: the copy is staged by the runtime and the call returns once the source may be reused
    if (hipMemcpyAsync(d, scalars_host, n * 32, hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess ||
        hipStreamSynchronize(ctx->c.stream) != hipSuccess) {
      ctx->c.pool.release(d);
      return BH_ERR_HIP;
    }
  }
  *out = new bh_scalars{ctx, d, n, scalar_fmt, true};
  return BH_OK;
}
int bh_scalars_adopt_dev(bh_ctx *ctx, void *scalars_dev, size_t n, int scalar_fmt, int take_ownership, bh_scalars **out) {
  if (!ctx || !out || (n && !scalars_dev)) return BH_ERR_INVALID_ARG;
  if (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT) return BH_ERR_INVALID_ARG;
  *out = new bh_scalars{ctx, scalars_dev, n, scalar_fmt, take_ownership != 0};
  return BH_OK;
}
void bh_scalars_release(bh_scalars *s) {
  if (!s) return;
  if (s->pooled) s->ctx->c.pool.release(s->dev);   // callers release after the multiexps that read it were waited on
  delete s;
}
size_t bh_scalars_len(const bh_scalars *s) { return s ? s->n : 0; }
const void *bh_scalars_dev_ptr(const bh_scalars *s) { return s ? s->dev : nullptr; }
int bh_msm_async_scalars(bh_ctx *ctx, const bh_bases *bases, size_t skip, const bh_scalars *scalars, size_t first,
                         size_t n, const uint64_t *density_words, size_t density_len, const bh_msm_opts *opts,
                         bh_msm_job **job) {
  if (!scalars || scalars->ctx != ctx || first > scalars->n || n > scalars->n - first) return BH_ERR_INVALID_ARG;
  // scalars on the device, density map on the host (a DensityTracker's words, 2^20 bits = 128 KiB)
  return msm_common(ctx, bases, skip, (const char *)scalars->dev + first * 32, false, n, scalars->fmt, density_words, true,
                    density_len, opts, job);
}
int bh_msm_async(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host, size_t n, int fmt,
                 const uint64_t *density_words, size_t density_len, bh_msm_job **job) {
  return msm_common(ctx, bases, skip, scalars_host, true, n, fmt, density_words, true, density_len, nullptr, job);
}
int bh_msm_async_opts(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host, size_t n, int fmt,
                      const uint64_t *density_words, size_t density_len, const bh_msm_opts *opts, bh_msm_job **job) {
  return msm_common(ctx, bases, skip, scalars_host, true, n, fmt, density_words, true, density_len, opts, job);
}
int bh_msm_async_dev(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t n, int fmt,
                     const uint64_t *density_words_dev, size_t density_len, bh_msm_job **job) {
  return msm_common(ctx, bases, skip, scalars_dev, false, n, fmt, density_words_dev, false, density_len, nullptr, job);
}
int bh_msm_async_dev_opts(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t n, int fmt,
                          const uint64_t *density_words_dev, size_t density_len, const bh_msm_opts *opts,
                          bh_msm_job **job) {
  return msm_common(ctx, bases, skip, scalars_dev, false, n, fmt, density_words_dev, false, density_len, opts, job);
}
// ---- one multiexp over several contexts of this process (one per GPU) -----------------------------
struct bh_msm_sharded_job {
  int group;
  std::vector<bh_msm_job *> jobs;                 // one per shard, in shard order
  std::vector<std::vector<uint64_t>> density;     // per-shard density words (re-based to bit 0), alive until the wait
};
int bh_msm_sharded_async(bh_ctx *const *ctxs, const bh_bases *const *shards, size_t n_shards, size_t skip,
                         const void *scalars_host, size_t n_scalars, int scalar_fmt, const uint64_t *density_words,
                         size_t density_len, bh_msm_sharded_job **out) {
  if (!ctxs || !shards || !n_shards || !out || (n_scalars && !scalars_host)) return BH_ERR_INVALID_ARG;
  if (density_words && density_len != n_scalars) return BH_ERR_INVALID_ARG;   // multiexp.rs:324-329
  for (size_t k = 0; k < n_shards; k++)
    if (!ctxs[k] || !shards[k] || shards[k]->group != shards[0]->group) return BH_ERR_INVALID_ARG;
  const int group = shards[0]->group;
  std::vector<size_t> lens(n_shards);
  for (size_t k = 0; k < n_shards; k++) lens[k] = shards[k]->n;
  std::vector<size_t> cut, off;
  shard_cuts(lens.data(), n_shards, skip, density_words, n_scalars, cut, off);
  std::unique_ptr<bh_msm_sharded_job> sj(new bh_msm_sharded_job());
  sj->group = group;
  sj->density.resize(n_shards);
  int rc = BH_OK;
  for (size_t k = 0; k < n_shards && rc == BH_OK; k++) {
    const size_t lo = cut[k], hi = cut[k + 1] > cut[k] ? cut[k + 1] : cut[k], n = hi - lo;
    // bases before the shard's first used record: only the shard that contains `skip` starts inside itself
    const size_t local_skip = skip > off[k] ? (skip - off[k] < shards[k]->n ? skip - off[k] : shards[k]->n) : 0;
    const uint64_t *dw = nullptr;
    if (density_words && n) {
      std::vector<uint64_t> &d = sj->density[k];
      d.assign((n + 63) / 64, 0);
      const size_t sh = lo & 63, w0 = lo >> 6, nw_all = (n_scalars + 63) / 64;
      for (size_t w = 0; w < d.size(); w++) {
        uint64_t x = density_words[w0 + w] >> sh;
        if (sh && w0 + w + 1 < nw_all) x |= density_words[w0 + w + 1] << (64 - sh);
        d[w] = x;
      }
      if (n & 63) d.back() &= (((uint64_t)1 << (n & 63)) - 1);
      dw = d.data();
    }
    bh_msm_job *j = nullptr;
    const bh_msm_opts o = {0, 0, BH_MSM_NO_SMALL_PATH};
    rc = msm_common(ctxs[k], shards[k], local_skip, (const char *)scalars_host + lo * 32, true, n, scalar_fmt, dw, true,
                    dw ? n : 0, &o, &j, n_scalars ? n_scalars : 1);
    if (rc == BH_OK) sj->jobs.push_back(j);
  }
  if (rc != BH_OK) {
    unsigned char sink[192];
    for (bh_msm_job *j : sj->jobs) (void)bh_msm_wait(j, sink);
    return rc;
  }
  *out = sj.release();
  return BH_OK;
}
int bh_msm_sharded_wait(bh_msm_sharded_job *job, void *out_affine) {
  if (!job || !out_affine) return BH_ERR_INVALID_ARG;
  const size_t rec = job->group == BH_G1 ? 96 : 192;
  alignas(16) unsigned char acc[192], part[192];
  memset(acc, 0, sizeof acc);
  // Error precedence of the whole multiexp from the shards': only the last shard can
  // reach the end of the bases, and every entry of an earlier shard precedes the first EOF entry, so an identity
  // consumed in the reference's top window by ANY shard wins over the EOF; without an EOF any identity is the error.
  bool hip_fail = false, eof = false, ident = false, ident_top = false;
  int other = BH_OK;
  for (size_t k = 0; k < job->jobs.size(); k++) {
    MsmJobImpl *impl = job->jobs[k]->impl;
    const int rc = msm_job_finish(*impl, part, nullptr);
    if (rc < 0) { hip_fail = true; other = rc; }
    eof |= impl->saw_eof;
    ident |= impl->saw_ident;
    // a shard that saw both resolves "top window, before its first EOF entry" itself
    ident_top |= impl->saw_ident_top;
    if (rc == BH_OK) host_point_add(job->group, acc, acc, part, 1);
    msm_job_delete(impl);
    delete job->jobs[k];
  }
  delete job;
  if (hip_fail) return other;
  if (eof && ident) return ident_top ? BH_ERR_UNEXPECTED_IDENTITY : BH_ERR_UNEXPECTED_EOF;
  if (eof) return BH_ERR_UNEXPECTED_EOF;
  if (ident) return BH_ERR_UNEXPECTED_IDENTITY;
  memcpy(out_affine, acc, rec);
  return BH_OK;
}

int bh_msm_async_dev_after(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t n, int fmt,
                           const uint64_t *density_words_dev, size_t density_len, const bh_msm_opts *opts, void *after_stream,
                           bh_msm_job **job) {
  if (!after_stream) return BH_ERR_INVALID_ARG;
  return msm_common(ctx, bases, skip, scalars_dev, false, n, fmt, density_words_dev, false, density_len, opts, job, 0,
                    after_stream);
}
int bh_msm_start(bh_msm_job *job) {
  if (!job) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(job->impl->ctx->device));
  return msm_job_start(*job->impl);
}
int bh_msm_wait_profile(bh_msm_job *job, void *out_affine, float *stage_ms4) {
  if (!job) return BH_ERR_INVALID_ARG;
  float ms[4] = {0, 0, 0, 0};
  int rc = msm_job_finish(*job->impl, out_affine, ms);
  if (stage_ms4) memcpy(stage_ms4, ms, sizeof ms);
  msm_job_delete(job->impl);
  delete job;
  return rc;
}
int bh_msm_wait_stats(bh_msm_job *job, void *out_affine, float *stage_ms4, uint64_t *stats8) {
  if (!job) return BH_ERR_INVALID_ARG;
  float ms[4] = {0, 0, 0, 0};
  u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = msm_job_finish(*job->impl, out_affine, ms, st);
  if (stage_ms4) memcpy(stage_ms4, ms, sizeof ms);
  if (stats8) memcpy(stats8, st, sizeof st);
  msm_job_delete(job->impl);
  delete job;
  return rc;
}
int bh_msm_plan_info(size_t n, int group, unsigned forced_c, unsigned *out9) {
  if (!out9 || (group != BH_G1 && group != BH_G2)) return BH_ERR_INVALID_ARG;
  const MsmPlan p = make_plan(n, forced_c, 0, group == BH_G2);
  out9[0] = p.c; out9[1] = p.W; out9[2] = p.nb; out9[3] = p.chunk; out9[4] = p.chunks_per_window; out9[5] = p.sort_passes;
  out9[6] = p.lo_bits; out9[7] = p.hi_bits; out9[8] = (unsigned)((u64)p.W * p.n);
  return BH_OK;
}
int bh_msm_debug_stages(bh_ctx *ctx, const void *scalars_host, size_t n, int scalar_fmt, unsigned c,
                        uint64_t *pairs_out_host, uint32_t *zstart_out_host) {
  if (!ctx || !scalars_host || !n || !pairs_out_host || !zstart_out_host) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  return msm_debug_stages(ctx->c, scalars_host, n, scalar_fmt, c, (u64 *)pairs_out_host, zstart_out_host);
}
int bh_msm_wait_timed(bh_msm_job *job, void *out_affine, float *device_ms) {
  float ms[4];
  int rc = bh_msm_wait_profile(job, out_affine, ms);
  if (device_ms) *device_ms = ms[0];
  return rc;
}
void bh_point_add(int group, void *r, const void *a, const void *b, size_t n) { host_point_add(group, r, a, b, n); }
int bh_msm_wait(bh_msm_job *job, void *out_affine) { return bh_msm_wait_timed(job, out_affine, nullptr); }

int bh_fixed_base_mul_dev(bh_ctx *ctx, int group, const void *base_affine_host, const void *scalars_dev, size_t n,
                          int fmt, void *out_dev, void *stream) {
  if (!ctx || (group != BH_G1 && group != BH_G2)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  // the window table of the base (32 x 255 affine records, built on the stream in front of the multiplications): a
  // plain allocation freed with hipFreeAsync-like semantics is not available for pool blocks, so it is a pool block
  // returned once the stream has drained - the call stays asynchronous for a caller-supplied stream only up to here
  hipStream_t st = pick_stream(ctx, stream);
  const size_t rec = group == BH_G1 ? 96 : 192;
  void *table = ctx->c.pool.acquire(FIXED_BASE_TABLE_RECORDS * rec);
  if (!table) return BH_ERR_HIP;
  int rc = fixed_base_mul(group, base_affine_host, scalars_dev, n, fmt, out_dev, st, table);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  ctx->c.pool.release(table);
  return rc;
}

int bh_point_mul_each_dev(bh_ctx *ctx, int group, const void *in_dev, const void *scalars_dev, size_t n, int scalar_fmt,
                          void *out_dev, void *stream) {
  if (!ctx || !group_ok(group) || (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT)) return BH_ERR_INVALID_ARG;
  if (!n) return BH_OK;
  if (!in_dev || !scalars_dev || !out_dev) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = pick_stream(ctx, stream);
  int rc = point_mul_each(group, in_dev, out_dev, n, scalars_dev, scalar_fmt, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  return rc;
}

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

void bh_point_mul(int group, void *r, const void *a, const void *k_canonical) { host_point_mul(group, r, a, k_canonical); }
void bh_point_lincomb(int group, void *r, const void *points, const void *scalars_canonical, size_t n) {
  host_point_lincomb(group, r, points, scalars_canonical, n);
}

}  // extern "C"
