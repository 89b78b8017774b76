// The handles behind the opaque types of include/bellman_hip.h and the few helpers the units of the C API share
// (api_context.hip, api_domain.hip, api_bases.hip, api_msm.hip; ceremony.hip reads a handle's group).
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "msm_types.hpp"

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
  bh::WindowTable tab = {0, 0, 0};
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
  bh::u32 table_stride = 0;   // bytes between the records of `table`
};
static inline bh::u32 dense_rec_bytes(int group) { return group == BH_G1 ? 96u : 192u; }
static inline size_t table_bytes(const bh_bases *b) { return b->table ? (size_t)b->tab.W * b->n * b->table_stride : 0; }
// ONE snapshot of a handle's sources for a job, under job_mu (the caller has reserved its job slot: bh_ctx_trim leaves
// tables alone while a call is issuing): the pointers and the strides they are read at come from the same moment - a
// trim + bh_bases_precompute between two reads of the handle could pair a freed table with the other stride
static inline bh::MsmBases bases_snapshot(bh_ctx *ctx, const bh_bases *b) {
  std::lock_guard<std::mutex> g(ctx->c.job_mu);
  bh::MsmBases s;
  s.dense = {b->dev, dense_rec_bytes(b->group)};
  if (b->padded) s.padded = {b->padded, 128u};
  if (b->table) s.table = {b->table, b->table_stride};
  s.tab = b->tab;
  s.n = b->n;
  return s;
}
// forgets the handle's automatic table in the context's books (caller holds job_mu; the table itself is the caller's to free)
static inline void forget_auto_table(bh_bases *b) {
  bh::Context &c = b->ctx->c;
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
  bh::MsmJobImpl *impl;
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

static inline hipStream_t pick_stream(bh_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->c.stream; }
static inline bool group_ok(int group) { return group == BH_G1 || group == BH_G2; }
