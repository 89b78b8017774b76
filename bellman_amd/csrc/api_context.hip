// Context, device memory and streams: entry points of include/bellman_hip.h.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "fft.hpp"
#include "handles.hpp"
#include "msm_job.hpp"

using namespace bh;

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

}  // extern "C"
