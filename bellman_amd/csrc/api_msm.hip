// Multiexp jobs - single, many-vector, sharded, over resident scalars - and the point-multiplication entry points of
// include/bellman_hip.h.
#include <string.h>

#include <algorithm>
#include <memory>
#include <thread>

#include "handles.hpp"
#include "msm_job.hpp"
#include "point_ops.hpp"
#include "points.hpp"
#include "shard_cuts.hpp"

using namespace bh;

extern "C" {

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

void bh_point_mul(int group, void *r, const void *a, const void *k_canonical) { host_point_mul(group, r, a, k_canonical); }
void bh_point_lincomb(int group, void *r, const void *points, const void *scalars_canonical, size_t n) {
  host_point_lincomb(group, r, points, scalars_canonical, n);
}

}  // extern "C"