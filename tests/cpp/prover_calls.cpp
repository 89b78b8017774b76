// The Groth16 prover host layer (csrc/groth16_prover.cpp, groth16_batch.cpp, groth16_callsites.cpp) calls only the C ABI of
// include/bellman_hip.h, so it runs here against a FAKE of that ABI - no GPU, no shared library.  The fake keeps a ledger
// (buffers, streams, jobs and what each job / queued stream operation was given pointers into) and a transcript of every
// call in a form free of addresses and scheduling.  Two things are held:
//   1. transcript: the calls of every scenario equal tests/cpp/prover_calls.expected.txt, which was recorded by this same
//      program in two parts.  Lines 1-1328 (host witnesses, up to the wrong-shaped witnesses): built against the csrc of the
//      commit BEFORE the prover paths were folded onto one multiexp table.  From line 1329 (the "dev ..." scenarios, witnesses
//      in device memory): built against the csrc of the commit BEFORE the grouped body of prove_witness_batch_dev_codes and
//      that of prove_witness_batch_codes were folded into one and the k-proof paths moved to groth16_batch.cpp; the first
//      part came out byte-identical in that recording.  Neither part is ever regenerated from later code: a line that
//      differs is a bug in the prover;
//   2. unwind: with each fallible call of a scenario made to fail in turn (issue / stream / memory calls with BH_ERR_HIP, a
//      job's wait with BH_ERR_UNEXPECTED_EOF, once more with an identity delta_g1 on top), every issued job is waited on
//      exactly once, every buffer is freed and every stream destroyed, no buffer is freed while an unwaited job or an
//      unsynchronised stream operation refers to it - and the code or exception equals the recorded one.  (The ledger is
//      an invariant of the code under test and not part of the record: the recorded commit itself left it dirty in 12 runs
//      - a failing allocation or upload of a host-evaluated proof's density maps freed the maps uploaded before it under
//      their queued uploads; the commit of the second part in 4 runs of "dev grouped, checked" - a failing upload, finish or
//      download of assemble_proofs freed its buffers under what was queued on the context's stream.)
// usage: prover_calls.bin EXPECTED        compare (exit 0 / 1)
//        prover_calls.bin --record FILE   write the transcript (only ever against the commits named above)
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bellman_hip.h"
#include "../../include/bellman_hip_test.h"
#include "../../bellman_amd/csrc/groth16_internal.hpp"

using groth16::Fr;

// ---- the fake's state ---------------------------------------------------------------------------------------------------
struct bh_ctx { int unused; };
struct bh_bases { int group; size_t n; const char *name; };
struct bh_msm_job { int group; std::string what; std::vector<int> refs; bool waited; };
struct bh_msm_many_job { int group; std::string what; size_t k; std::vector<int> refs; bool waited; };
struct bh_scalars { size_t n; int region; void *mem; };
struct bh_r1cs {
  size_t n_in, n_aux, n_cons;
  const uint64_t *host[3];
  uint64_t *dev[3];
  size_t b_in_total;
};

namespace {
enum Kind { PLAIN = 0, ISSUE = 1, WAIT = 2 };
// dev: a device buffer - pointers into it are bounds-checked and tracked in a job's / a stream's references.  callers: a
// device buffer that belongs to the caller of the prover (resident witnesses): tracked like any other, so that a buffer of
// the proof freed under a job that also reads the caller's stays findable, but never freed by the prover and not counted
// as "never freed".
struct Region { int id; size_t size; std::string name; bool dev; bool callers = false; };
struct Stream { std::vector<int> pending; bool live = true; };
struct Fallible { std::string line; int occ; int kind; };

std::mutex mu;
bool quiet = false;   // set-up and tear-down of a scenario's fixtures: neither recorded nor failed
std::map<uintptr_t, Region> regions;
int next_region = 0;
std::vector<std::unique_ptr<Stream>> streams;
Stream ctx_stream;
std::vector<std::unique_ptr<bh_msm_job>> jobs;
std::vector<std::unique_ptr<bh_msm_many_job>> many_jobs;
std::vector<std::string> violations, main_log, helper_log;
std::thread::id main_id;
std::map<std::string, int> seen;
std::vector<Fallible> fallible, fallible_helper;   // the main thread's in call order; the helpers' are sorted before use
std::string fail_line;
int fail_occ = -1;
std::vector<uint32_t> check_answers;   // what bh_r1cs_check_many_dev answers, witness by witness across its calls
size_t check_next = 0;
int bases_made = 0;

std::string fmt(const char *f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
int note(const std::string &line, int kind) {
  if (quiet) return BH_OK;
  (std::this_thread::get_id() == main_id ? main_log : helper_log).push_back(line);
  if (kind == PLAIN) return BH_OK;
  const int occ = seen[line]++;
  (std::this_thread::get_id() == main_id ? fallible : fallible_helper).push_back(Fallible{line, occ, kind});
  if (line == fail_line && occ == fail_occ) return kind == ISSUE ? BH_ERR_HIP : BH_ERR_UNEXPECTED_EOF;
  return BH_OK;
}
Region *region_of(const void *p, size_t *off) {
  auto it = regions.upper_bound((uintptr_t)p);
  if (it == regions.begin()) return nullptr;
  --it;
  if ((uintptr_t)p > it->first + it->second.size) return nullptr;
  *off = (uintptr_t)p - it->first;
  return &it->second;
}
// a pointer as "<region>[<bytes>]+<offset>"; device regions it points into are added to `refs`
std::string P(const void *p, std::vector<int> *refs = nullptr) {
  if (!p) return "null";
  size_t off = 0;
  Region *r = region_of(p, &off);
  if (!r) return "host";
  if (refs && r->dev) refs->push_back(r->id);
  return fmt("%s[%zu]+%zu", r->name.c_str(), r->size, off);
}
void *add_region(size_t bytes, const char *name, bool dev, bool callers = false) {
  void *p = malloc(bytes ? bytes : 1);
  regions[(uintptr_t)p] = Region{next_region++, bytes, name, dev, callers};
  return p;
}
void name_host(const char *name, const void *p, size_t bytes) {
  std::lock_guard<std::mutex> g(mu);
  regions[(uintptr_t)p] = Region{next_region++, bytes, name, false};
}
// the bytes [p, p + n) lie inside one device buffer
bool in_bounds(const void *p, size_t n, const char *what) {
  size_t off = 0;
  Region *r = region_of(p, &off);
  if (r && r->dev && off + n <= r->size) return true;
  violations.push_back(fmt("%s: %zu bytes at %s leave the buffer", what, n, P(p).c_str()));
  return false;
}
void drop_region(void *p, const char *what) {
  auto it = regions.find((uintptr_t)p);
  if (it == regions.end()) { violations.push_back(fmt("%s of an unknown buffer", what)); return; }
  const int id = it->second.id;
  for (auto &j : jobs)
    if (!j->waited && std::count(j->refs.begin(), j->refs.end(), id)) violations.push_back(fmt("%s under an unwaited job: %s[%zu]", what, it->second.name.c_str(), it->second.size));
  for (auto &j : many_jobs)
    if (!j->waited && std::count(j->refs.begin(), j->refs.end(), id)) violations.push_back(fmt("%s under an unwaited many-job: %s[%zu]", what, it->second.name.c_str(), it->second.size));
  auto pending = [&](Stream &s) { return std::count(s.pending.begin(), s.pending.end(), id) != 0; };
  bool queued = pending(ctx_stream);
  for (auto &s : streams) queued = queued || pending(*s);
  if (queued) violations.push_back(fmt("%s under an unsynchronised stream operation: %s[%zu]", what, it->second.name.c_str(), it->second.size));
  regions.erase(it);
  free(p);
}
Stream *stream_of(void *st) { return st ? (Stream *)st : &ctx_stream; }
const char *S(void *st) { return st ? "stream" : "ctx-stream"; }
void queue_on(void *st, const std::vector<int> &refs) {
  Stream *s = stream_of(st);
  if (!s->live) violations.push_back("operation queued on a destroyed stream");
  s->pending.insert(s->pending.end(), refs.begin(), refs.end());
}
int issue_job(const std::string &line, const bh_bases *b, size_t n, std::vector<int> refs, bh_msm_job **job) {
  if (int rc = note(line, ISSUE)) return rc;
  jobs.emplace_back(new bh_msm_job{b->group, fmt("%s n=%zu", b->name, n), std::move(refs), false});
  *job = jobs.back().get();
  return BH_OK;
}
}  // namespace

// ---- the fake C ABI (only what the scenarios reach; the linker leaves the rest of the header unresolved) ------------------
#define LOCK std::lock_guard<std::mutex> lock_(mu)
extern "C" {
int bh_dev_alloc(bh_ctx *, size_t bytes, void **out) {
  LOCK;
  if (int rc = note(fmt("bh_dev_alloc %zu", bytes), ISSUE)) return rc;
  *out = add_region(bytes, "dev", true);
  return BH_OK;
}
int bh_dev_free(bh_ctx *, void *p) {
  LOCK;
  note(fmt("bh_dev_free %s", P(p).c_str()), PLAIN);
  drop_region(p, "bh_dev_free");
  return BH_OK;
}
static int upload(const char *name, void *dst, const void *src, size_t bytes, void *st) {
  std::vector<int> refs;
  const std::string line = fmt("%s %s <- %s %zu %s", name, P(dst, &refs).c_str(), P(src).c_str(), bytes, S(st));
  if (int rc = note(line, ISSUE)) return rc;
  if (in_bounds(dst, bytes, name)) memcpy(dst, src, bytes);
  queue_on(st, refs);
  return BH_OK;
}
int bh_dev_upload(bh_ctx *, void *dst, const void *src, size_t bytes) { LOCK; return upload("bh_dev_upload", dst, src, bytes, nullptr); }
int bh_dev_upload_on(bh_ctx *, void *dst, const void *src, size_t bytes, void *st) { LOCK; return upload("bh_dev_upload_on", dst, src, bytes, st); }
int bh_dev_download(bh_ctx *, void *dst, const void *src, size_t bytes) {
  LOCK;
  if (int rc = note(fmt("bh_dev_download %s <- %s %zu", P(dst).c_str(), P(src).c_str(), bytes), ISSUE)) return rc;
  if (in_bounds(src, bytes, "bh_dev_download")) memcpy(dst, src, bytes);
  ctx_stream.pending.clear();   // it synchronises the context stream
  return BH_OK;
}
static int zero(const char *name, void *p, size_t bytes, void *st) {
  std::vector<int> refs;
  if (int rc = note(fmt("%s %s %zu %s", name, P(p, &refs).c_str(), bytes, S(st)), ISSUE)) return rc;
  if (in_bounds(p, bytes, name)) memset(p, 0, bytes);
  queue_on(st, refs);
  return BH_OK;
}
int bh_dev_zero(bh_ctx *, void *p, size_t bytes) { LOCK; return zero("bh_dev_zero", p, bytes, nullptr); }
int bh_dev_zero_on(bh_ctx *, void *p, size_t bytes, void *st) { LOCK; return zero("bh_dev_zero_on", p, bytes, st); }
int bh_stream_create_priority(bh_ctx *, int high, void **out) {
  LOCK;
  if (int rc = note(fmt("bh_stream_create_priority %d", high), ISSUE)) return rc;
  streams.emplace_back(new Stream());
  *out = streams.back().get();
  return BH_OK;
}
int bh_stream_destroy(bh_ctx *, void *st) {
  LOCK;
  note("bh_stream_destroy", PLAIN);
  Stream *s = stream_of(st);
  if (!s->live) violations.push_back("stream destroyed twice");
  if (!s->pending.empty()) violations.push_back("stream destroyed with operations queued");
  s->live = false;
  return BH_OK;
}
int bh_stream_synchronize(bh_ctx *, void *st) {
  LOCK;
  const int rc = note(fmt("bh_stream_synchronize %s", S(st)), ISSUE);
  stream_of(st)->pending.clear();   // (a failing synchronise has still waited: the device is the one that failed)
  return rc;
}
int bh_ctx_synchronize(bh_ctx *) {
  LOCK;
  const int rc = note("bh_ctx_synchronize", ISSUE);
  ctx_stream.pending.clear();
  for (auto &s : streams) s->pending.clear();
  return rc;
}
int bh_ctx_accumulations_after(bh_ctx *, void *st) { LOCK; return note(fmt("bh_ctx_accumulations_after %s", S(st)), ISSUE); }
int bh_fft_fr(bh_ctx *, void *, uint32_t log_n, int mode) { LOCK; return note(fmt("bh_fft_fr host log_n=%u mode=%d", log_n, mode), ISSUE); }
int bh_fft_fr_dev(bh_ctx *, void *d, uint32_t log_n, int mode, void *st) {
  LOCK;
  std::vector<int> refs;
  if (int rc = note(fmt("bh_fft_fr_dev %s log_n=%u mode=%d %s", P(d, &refs).c_str(), log_n, mode, S(st)), ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
static int pointwise(const char *name, void *a, const void *b, size_t n, void *st) {
  std::vector<int> refs;
  if (int rc = note(fmt("%s %s %s n=%zu %s", name, P(a, &refs).c_str(), P(b, &refs).c_str(), n, S(st)), ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
int bh_fr_mul_assign_dev(bh_ctx *, void *a, const void *b, size_t n, void *st) { LOCK; return pointwise("bh_fr_mul_assign_dev", a, b, n, st); }
int bh_fr_sub_assign_dev(bh_ctx *, void *a, const void *b, size_t n, void *st) { LOCK; return pointwise("bh_fr_sub_assign_dev", a, b, n, st); }
int bh_fr_divide_by_z_on_coset_dev(bh_ctx *, void *a, uint32_t log_n, void *st) { LOCK; return pointwise("bh_fr_divide_by_z_on_coset_dev", a, nullptr, log_n, st); }
int bh_h_poly_fr_dev_on(bh_ctx *, void *a, void *b, void *c, void *scratch, uint32_t log_n, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_h_poly_fr_dev_on %s %s %s scratch=%s log_n=%u %s", P(a, &refs).c_str(), P(b, &refs).c_str(),
                               P(c, &refs).c_str(), P(scratch, &refs).c_str(), log_n, S(st));
  if (int rc = note(line, ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
int bh_h_poly_fr_many_dev_on(bh_ctx *, void *a, void *b, void *c, size_t stride, size_t k, uint32_t log_n, unsigned flags,
                             void *scratch, size_t scratch_bytes, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_h_poly_fr_many_dev_on %s %s %s stride=%zu k=%zu log_n=%u flags=%u scratch=%s %zu %s", P(a, &refs).c_str(),
                               P(b, &refs).c_str(), P(c, &refs).c_str(), stride, k, log_n, flags, P(scratch, &refs).c_str(), scratch_bytes, S(st));
  if (int rc = note(line, ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
int bh_bases_register(bh_ctx *, int group, const void *, size_t n, size_t, long, bh_bases **out) {
  LOCK;
  static const char *names[5] = {"h", "l", "a", "b_g1", "b_g2"};   // the order Parameters registers them in
  *out = new bh_bases{group, n, names[bases_made++ % 5]};
  return BH_OK;
}
void bh_bases_release(bh_ctx *, bh_bases *b) { delete b; }
size_t bh_bases_len(const bh_bases *b) { return b->n; }
int bh_msm_async(bh_ctx *, const bh_bases *b, size_t skip, const void *scalars, size_t n, int f, const uint64_t *dens, size_t dens_len,
                 bh_msm_job **job) {
  LOCK;
  return issue_job(fmt("bh_msm_async %s skip=%zu scalars=%s n=%zu fmt=%d density=%s %zu", b->name, skip, P(scalars).c_str(), n, f,
                       P(dens).c_str(), dens_len), b, n, {}, job);
}
int bh_msm_async_dev(bh_ctx *, const bh_bases *b, size_t skip, const void *scalars, size_t n, int f, const uint64_t *dens,
                     size_t dens_len, bh_msm_job **job) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_msm_async_dev %s skip=%zu scalars=%s n=%zu fmt=%d density=%s %zu", b->name, skip, P(scalars, &refs).c_str(),
                               n, f, P(dens, &refs).c_str(), dens_len);
  return issue_job(line, b, n, refs, job);
}
int bh_msm_async_dev_after(bh_ctx *, const bh_bases *b, size_t skip, const void *scalars, size_t n, int f, const uint64_t *dens,
                           size_t dens_len, const bh_msm_opts *opts, void *after, bh_msm_job **job) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_msm_async_dev_after %s skip=%zu scalars=%s n=%zu fmt=%d density=%s %zu opts=%s after=%s", b->name, skip,
                               P(scalars, &refs).c_str(), n, f, P(dens, &refs).c_str(), dens_len, opts ? "set" : "null", S(after));
  return issue_job(line, b, n, refs, job);
}
int bh_msm_async_scalars(bh_ctx *, const bh_bases *b, size_t skip, const bh_scalars *sc, size_t first, size_t n, const uint64_t *dens,
                         size_t dens_len, const bh_msm_opts *opts, bh_msm_job **job) {
  LOCK;
  const std::string line = fmt("bh_msm_async_scalars %s skip=%zu scalars[%zu] first=%zu n=%zu density=%s %zu opts=%s", b->name, skip, sc->n,
                               first, n, P(dens).c_str(), dens_len, opts ? "set" : "null");
  return issue_job(line, b, n, {sc->region}, job);
}
int bh_msm_wait(bh_msm_job *job, void *out) {
  LOCK;
  const int rc = note(fmt("bh_msm_wait %s", job->what.c_str()), WAIT);
  if (job->waited) violations.push_back("a job waited on twice");
  job->waited = true;
  memset(out, 0, job->group == BH_G1 ? 96 : 192);   // the identity record
  return rc;
}
int bh_msm_many_async_dev(bh_ctx *, const bh_bases *b, size_t skip, const void *scalars, size_t stride, size_t n, size_t k, int f,
                          const uint64_t *dens, size_t dens_len, const bh_msm_opts *opts, void *after, bh_msm_many_job **job) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_msm_many_async_dev %s skip=%zu scalars=%s stride=%zu n=%zu k=%zu fmt=%d density=%s %zu opts=%s after=%s",
                               b->name, skip, P(scalars, &refs).c_str(), stride, n, k, f, P(dens, &refs).c_str(), dens_len,
                               opts ? "set" : "null", S(after));
  if (int rc = note(line, ISSUE)) return rc;
  many_jobs.emplace_back(new bh_msm_many_job{b->group, fmt("%s n=%zu", b->name, n), k, refs, false});
  *job = many_jobs.back().get();
  return BH_OK;
}
int bh_msm_many_wait(bh_msm_many_job *job, void *out, int32_t *rcs, float *, uint64_t *) {
  LOCK;
  const int rc = note(fmt("bh_msm_many_wait %s k=%zu out=%s", job->what.c_str(), job->k, out ? "set" : "null"), WAIT);
  if (job->waited) violations.push_back("a many-job waited on twice");
  job->waited = true;
  if (out) memset(out, 0, job->k * (job->group == BH_G1 ? 96 : 192));
  if (rcs) {   // a failing wait is the FIRST vector's: the per-proof codes are what the prover sorts out
    for (size_t j = 0; j < job->k; j++) rcs[j] = BH_OK;
    rcs[0] = rc;
  }
  return BH_OK;
}
void bh_point_add(int group, void *r, const void *, const void *, size_t n) {
  LOCK;
  note(fmt("bh_point_add g%d n=%zu", group, n), PLAIN);
  memset(r, 0, n * (group == BH_G1 ? 96 : 192));
}
void bh_point_mul(int group, void *r, const void *, const void *) {
  LOCK;
  note(fmt("bh_point_mul g%d", group), PLAIN);
  memset(r, 0, group == BH_G1 ? 96 : 192);
}
void bh_point_lincomb(int group, void *r, const void *, const void *scalars, size_t n) {
  LOCK;
  note(fmt("bh_point_lincomb g%d n=%zu scalars=%s", group, n, scalars ? "set" : "ones"), PLAIN);
  memset(r, 0, group == BH_G1 ? 96 : 192);
}
int bh_scalars_register(bh_ctx *, const void *src, size_t n, int f, bh_scalars **out) {
  LOCK;
  if (int rc = note(fmt("bh_scalars_register %s n=%zu fmt=%d", P(src).c_str(), n, f), ISSUE)) return rc;
  void *mem = add_region(n * 32, "scalars", true);
  *out = new bh_scalars{n, regions[(uintptr_t)mem].id, mem};
  return BH_OK;
}
void bh_scalars_release(bh_scalars *s) {
  LOCK;
  note(fmt("bh_scalars_release scalars[%zu]", s->n), PLAIN);
  drop_region(s->mem, "bh_scalars_release");
  delete s;
}
size_t bh_scalars_len(const bh_scalars *s) { return s->n; }
int bh_h_poly_fr_scalars(bh_ctx *, const void *a, const void *b, const void *c, size_t n, bh_scalars **out) {
  LOCK;
  if (int rc = note(fmt("bh_h_poly_fr_scalars %s %s %s n=%zu", P(a).c_str(), P(b).c_str(), P(c).c_str(), n), ISSUE)) return rc;
  size_t m = 1;
  while (m < n) m *= 2;
  void *mem = add_region((m - 1) * 32, "scalars", true);
  *out = new bh_scalars{m - 1, regions[(uintptr_t)mem].id, mem};
  return BH_OK;
}
int bh_r1cs_shape(const bh_r1cs *r, size_t *n_in, size_t *n_aux, size_t *n_cons) {
  *n_in = r->n_in; *n_aux = r->n_aux; *n_cons = r->n_cons;
  return BH_OK;
}
void bh_r1cs_release(bh_r1cs *) {}
int bh_r1cs_density(const bh_r1cs *r, int which, const uint64_t **dev, const uint64_t **host, size_t *total) {
  LOCK;
  if (int rc = note(fmt("bh_r1cs_density %d total=%s", which, total ? "asked" : "null"), ISSUE)) return rc;
  if (dev) *dev = r->dev[which];
  if (host) *host = r->host[which];
  if (total) *total = r->b_in_total;
  return BH_OK;
}
int bh_r1cs_eval_dev(bh_ctx *, const bh_r1cs *, const void *in, const void *aux, void *a, void *b, void *c, uint32_t log_m, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_r1cs_eval_dev in=%s aux=%s -> %s %s %s log_m=%u %s", P(in, &refs).c_str(), P(aux, &refs).c_str(),
                               P(a, &refs).c_str(), P(b, &refs).c_str(), P(c, &refs).c_str(), log_m, S(st));
  if (int rc = note(line, ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
int bh_r1cs_eval_many_dev(bh_ctx *, const bh_r1cs *, const void *in, size_t in_stride, const void *aux, size_t aux_stride, size_t k, void *a,
                          void *b, void *c, size_t out_stride, uint32_t log_m, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_r1cs_eval_many_dev in=%s %zu aux=%s %zu k=%zu -> %s %s %s %zu log_m=%u %s", P(in, &refs).c_str(), in_stride,
                               P(aux, &refs).c_str(), aux_stride, k, P(a, &refs).c_str(), P(b, &refs).c_str(), P(c, &refs).c_str(),
                               out_stride, log_m, S(st));
  if (int rc = note(line, ISSUE)) return rc;
  queue_on(st, refs);
  return BH_OK;
}
int bh_r1cs_check_many_dev(bh_ctx *, const bh_r1cs *, const void *in, size_t in_stride, const void *aux, size_t aux_stride, size_t k,
                           uint32_t *bad, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_r1cs_check_many_dev in=%s %zu aux=%s %zu k=%zu -> %s %s", P(in, &refs).c_str(), in_stride,
                               P(aux, &refs).c_str(), aux_stride, k, P(bad, &refs).c_str(), S(st));
  if (int rc = note(line, ISSUE)) return rc;
  if (in_bounds(bad, k * 4, "bh_r1cs_check_many_dev"))
    for (size_t j = 0; j < k; j++) bad[j] = check_next < check_answers.size() ? check_answers[check_next++] : BH_R1CS_SATISFIED;
  queue_on(st, refs);
  return BH_OK;
}
int bh_proof_finish_dev(bh_ctx *, const void *vk5, const void *sums, const void *r, const void *s, size_t k, void *proofs, void *st) {
  LOCK;
  std::vector<int> refs;
  const std::string line = fmt("bh_proof_finish_dev vk5=%s sums=%s r=%s s=%s k=%zu -> %s %s", P(vk5).c_str(), P(sums, &refs).c_str(),
                               P(r, &refs).c_str(), P(s, &refs).c_str(), k, P(proofs, &refs).c_str(), S(st));
  if (int rc = note(line, ISSUE)) return rc;
  in_bounds(sums, k * BH_MSM_SUMS_BYTES, "bh_proof_finish_dev");
  in_bounds(r, k * 32, "bh_proof_finish_dev");
  in_bounds(s, k * 32, "bh_proof_finish_dev");
  if (in_bounds(proofs, k * 384, "bh_proof_finish_dev")) memset(proofs, 0, k * 384);
  queue_on(st, refs);
  return BH_OK;
}
}  // extern "C"

// ---- fixtures -------------------------------------------------------------------------------------------------------------
namespace {
struct Quiet {
  Quiet() { std::lock_guard<std::mutex> g(mu); quiet = true; }
  ~Quiet() { std::lock_guard<std::mutex> g(mu); quiet = false; }
};
bh_ctx the_ctx;

// one circuit shape with k witnesses, the evaluations of witness 0, density maps and parameters.  `gap` Fr between the
// witnesses' host vectors (0: each starts where the one before ends)
struct World {
  size_t n_in, n_aux, n_cons, k, gap;
  std::vector<Fr> inputs, aux, a, b, c, r, s;
  std::vector<uint64_t> dens[3];
  bh_r1cs r1cs;
  std::unique_ptr<groth16::Parameters> params;
  std::unique_ptr<groth16::R1cs> shape;
  std::vector<groth16::WitnessView> views;
  void *dev_inputs = nullptr, *dev_aux = nullptr;   // the caller's device buffers (resident)
  World(size_t n_in_, size_t n_aux_, size_t n_cons_, size_t k_ = 1, size_t gap_ = 0, bool identity_delta = false)
      : n_in(n_in_), n_aux(n_aux_), n_cons(n_cons_), k(k_), gap(gap_) {
    Quiet q;
    auto fill = [](std::vector<Fr> &v, size_t n, uint64_t from) { v.resize(n); for (size_t i = 0; i < n; i++) v[i] = Fr::from_u64(from + i); };
    fill(inputs, k * (n_in + gap), 1); fill(aux, k * (n_aux + gap), 1000);
    fill(a, n_cons, 3); fill(b, n_cons, 5); fill(c, n_cons, 7);
    fill(r, k, 11); fill(s, k, 13);
    // density maps with zeros in every word: a multiexp's base offset is a popcount, not an index
    dens[0].assign((n_aux + 63) / 64, 0xFFFF00FFF0F0FFFFull);
    dens[1].assign((n_in + 63) / 64, 0x00000000000001EDull);
    dens[2].assign((n_aux + 63) / 64, 0x0F0F0F0F0F0FFFF0ull);
    name_host("inputs", inputs.data(), inputs.size() * 32); name_host("aux", aux.data(), aux.size() * 32);
    name_host("a", a.data(), n_cons * 32); name_host("b", b.data(), n_cons * 32); name_host("c", c.data(), n_cons * 32);
    static const char *host_names[3] = {"a_aux_density", "b_input_density", "b_aux_density"};
    static const char *dev_names[3] = {"dev_a_aux_density", "dev_b_input_density", "dev_b_aux_density"};
    r1cs.n_in = n_in; r1cs.n_aux = n_aux; r1cs.n_cons = n_cons;
    for (int i = 0; i < 3; i++) {
      name_host(host_names[i], dens[i].data(), dens[i].size() * 8);
      r1cs.host[i] = dens[i].data();
      std::lock_guard<std::mutex> g(mu);
      r1cs.dev[i] = (uint64_t *)add_region(dens[i].size() * 8, dev_names[i], false);   // the handle's: not a buffer of the proof
    }
    r1cs.b_in_total = 0;
    for (size_t i = 0; i < n_in; i++) r1cs.b_in_total += (dens[1][i / 64] >> (i & 63)) & 1;
    groth16::VerifyingKey vk;
    memset((void *)&vk.alpha_g1, 1, sizeof vk.alpha_g1); memset((void *)&vk.beta_g1, 1, sizeof vk.beta_g1);
    memset((void *)&vk.beta_g2, 1, sizeof vk.beta_g2); memset((void *)&vk.delta_g2, 1, sizeof vk.delta_g2);
    memset((void *)&vk.delta_g1, identity_delta ? 0 : 1, sizeof vk.delta_g1);
    groth16::G1Affine g1{};
    groth16::G2Affine g2{};
    params.reset(new groth16::Parameters(&the_ctx, vk, &g1, 1, &g1, 1, &g1, 1, &g1, 1, &g2, 1));
    shape.reset(new groth16::R1cs(&r1cs, &the_ctx));
    for (size_t j = 0; j < k; j++)
      views.push_back(groth16::WitnessView{inputs.data() + j * (n_in + gap), n_in, aux.data() + j * (n_aux + gap), n_aux});
  }
  ~World() {
    Quiet q;
    shape.reset();
    params.reset();
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < 3; i++) free(r1cs.dev[i]);
    free(dev_inputs);
    free(dev_aux);
    regions.clear();
  }
  // the k witnesses once more in two caller-owned device buffers, `pad` bytes between one vector's end and the next
  groth16::DeviceWitnesses resident(size_t pad) {
    Quiet q;
    std::lock_guard<std::mutex> g(mu);
    const size_t in_stride = n_in * 32 + pad, aux_stride = n_aux * 32 + pad;
    dev_inputs = add_region(k * in_stride, "dev_inputs", true, true);
    dev_aux = add_region(k * aux_stride, "dev_aux", true, true);
    memset(dev_inputs, 0, k * in_stride);
    memset(dev_aux, 0, k * aux_stride);
    for (size_t j = 0; j < k; j++) {
      memcpy((char *)dev_inputs + j * in_stride, (const void *)views[j].inputs, n_in * 32);
      memcpy((char *)dev_aux + j * aux_stride, (const void *)views[j].aux, n_aux * 32);
    }
    return groth16::DeviceWitnesses{dev_inputs, in_stride, dev_aux, aux_stride, k};
  }
  groth16::AssignmentView assignment() const {
    return groth16::AssignmentView{a.data(), b.data(), c.data(), n_cons, inputs.data(), n_in, aux.data(), n_aux,
                                   dens[0].data(), dens[1].data(), dens[2].data()};
  }
};

std::string codes_text(const std::vector<int> &codes) {
  std::string t = " codes";
  for (int x : codes) t += fmt(" %d", x);
  return t;
}
// what a scenario's body did, as the caller sees it
std::string outcome_of(const std::function<std::string()> &body) {
  try {
    return "ok" + body();
  } catch (const bellman::SynthesisError &e) { return fmt("SynthesisError(%d)", e.code);
  } catch (const std::invalid_argument &) { return "invalid_argument";
  } catch (const std::runtime_error &) { return "runtime_error";
  } catch (...) { return "another exception"; }
}

struct Scenario {
  std::string name;
  bool sweep;
  // builds its World (identity delta on request), runs the prover, returns the outcome
  std::function<std::string(bool identity_delta)> run;
};

std::string ledger() {
  std::lock_guard<std::mutex> g(mu);
  std::vector<std::string> v = violations;
  size_t unwaited = 0, live_streams = 0, live_buffers = 0;
  for (auto &j : jobs) unwaited += !j->waited;
  for (auto &j : many_jobs) unwaited += !j->waited;
  for (auto &s : streams) live_streams += s->live;
  for (auto &r : regions) live_buffers += r.second.dev && !r.second.callers;
  if (unwaited) v.push_back(fmt("%zu jobs never waited on", unwaited));
  if (live_streams) v.push_back(fmt("%zu streams never destroyed", live_streams));
  if (live_buffers) v.push_back(fmt("%zu buffers never freed", live_buffers));
  std::string t;
  for (const std::string &x : v) t += " [" + x + "]";
  return t;
}
// The ledger is an invariant of the code under test, not part of the record: a run that leaves it dirty is listed here.
std::vector<std::string> dirty;
std::string running;   // the scenario and the failing call, for that list
void close_ledger() {
  const std::string l = ledger();
  if (!l.empty()) dirty.push_back(running + ":" + l);
}
// the outcome and the ledger, read while the scenario's World (the region table) is still alive
std::string ledgered(const World &, const std::function<std::string()> &body) {
  const std::string outcome = outcome_of(body);
  close_ledger();
  return outcome;
}
void reset(const std::string &line, int occ) {
  std::lock_guard<std::mutex> g(mu);
  streams.clear(); jobs.clear(); many_jobs.clear(); violations.clear(); main_log.clear(); helper_log.clear(); seen.clear();
  fallible.clear(); fallible_helper.clear(); ctx_stream.pending.clear(); check_answers.clear();
  check_next = 0; bases_made = 0; next_region = 0;
  main_id = std::this_thread::get_id();
  fail_line = line; fail_occ = occ;
}

// a run of equal consecutive lines is written once, with its length
void print_calls(std::ostream &out, const char *who, const std::vector<std::string> &log) {
  for (size_t i = 0, j; i < log.size(); i = j) {
    for (j = i + 1; j < log.size() && log[j] == log[i]; j++) {}
    out << who << log[i];
    if (j - i > 1) out << "   (x" << j - i << ")";
    out << "\n";
  }
}

void play(const Scenario &sc, std::ostream &out) {
  reset("", -1);
  running = sc.name;
  const std::string outcome = sc.run(false);
  out << "== " << sc.name << "\n";
  std::sort(helper_log.begin(), helper_log.end());
  print_calls(out, "main   ", main_log);
  print_calls(out, "helper ", helper_log);
  out << "-> " << outcome << "\n";
  if (!sc.sweep) return;
  std::vector<Fallible> calls = fallible;
  std::sort(fallible_helper.begin(), fallible_helper.end(), [](const Fallible &x, const Fallible &y) { return x.line != y.line ? x.line < y.line : x.occ < y.occ; });
  calls.insert(calls.end(), fallible_helper.begin(), fallible_helper.end());
  // every fallible call fails once, the main thread's in call order, then the helpers' sorted; runs of consecutive calls
  // with one outcome are written as one line that names the first and the last of them
  int first_wait = -1;
  std::vector<std::string> outcomes;
  for (size_t i = 0; i < calls.size(); i++) {
    if (calls[i].kind == WAIT && first_wait < 0) first_wait = (int)i;
    reset(calls[i].line, calls[i].occ);
    running = sc.name + ", failing " + calls[i].line + fmt(" #%d", calls[i].occ);
    outcomes.push_back(sc.run(false));
  }
  for (size_t i = 0, j; i < calls.size(); i = j) {
    for (j = i + 1; j < calls.size() && outcomes[j] == outcomes[i]; j++) {}
    out << "fail " << i << ": " << calls[i].line << " #" << calls[i].occ;
    if (j - i > 1) out << " .. " << j - 1 << ": " << calls[j - 1].line << " #" << calls[j - 1].occ;
    out << " -> " << outcomes[i] << "\n";
  }
  if (first_wait >= 0) {
    reset(calls[first_wait].line, calls[first_wait].occ);
    running = sc.name + ", identity delta_g1, failing " + calls[first_wait].line;
    const std::string o = sc.run(true);
    out << "fail " << calls[first_wait].line << " #" << calls[first_wait].occ << " with an identity delta_g1 -> " << o << "\n";
  }
}

constexpr size_t N_AUX = 200;   // three density words and a ragged fourth
Scenario single(const char *name, bool host, size_t n_in, size_t n_cons) {
  return Scenario{name, true, [=](bool idd) {
    World w(n_in, N_AUX, n_cons, 1, 0, idd);
    return ledgered(w, [&] {
      if (host) groth16::prove_assignment(w.assignment(), *w.params, w.r[0], w.s[0]);
      else groth16::prove_witness(*w.shape, *w.params, w.inputs.data(), n_in, w.aux.data(), N_AUX, w.r[0], w.s[0]);
      return std::string();
    });
  }};
}
Scenario batch(const char *name, int mode, size_t k, size_t budget, size_t gap, bool checked, bool sweep) {
  return Scenario{name, sweep, [=](bool idd) {
    World w(2, N_AUX, 13, k, gap, idd);
    if (checked) check_answers = {BH_R1CS_SATISFIED, BH_R1CS_SATISFIED, 7, BH_R1CS_SATISFIED};
    std::vector<groth16::Proof> proofs(k);
    std::vector<int> codes(k, -99);
    std::vector<uint32_t> bad(k, 0);
    return ledgered(w, [&] {
      if (checked)
        groth16::prove_witness_batch_checked_codes(*w.shape, *w.params, w.views.data(), k, w.r.data(), w.s.data(), proofs.data(),
                                                   codes.data(), bad.data(), nullptr, budget, mode);
      else
        groth16::prove_witness_batch_codes(*w.shape, *w.params, w.views.data(), k, w.r.data(), w.s.data(), proofs.data(), codes.data(),
                                           nullptr, budget, mode);
      std::string t = codes_text(codes);
      if (checked) { t += " first_unsatisfied"; for (uint32_t x : bad) t += fmt(" %u", x); }
      return t;
    });
  }};
}
Scenario call_sites(const char *name, int mode) {
  return Scenario{name, true, [=](bool idd) {
    World w(2, N_AUX, 13, 1, 0, idd);
    bh_params handle{w.params.get()};
    unsigned char proof[384];
    const int rc = bh_test_groth16_prove_via_call_sites(&handle, mode, w.a.data(), w.b.data(), w.c.data(), w.n_cons, w.inputs.data(), w.n_in,
                                                        w.aux.data(), w.n_aux, w.dens[0].data(), w.dens[1].data(), w.dens[2].data(),
                                                        &w.r[0], &w.s[0], proof, nullptr);
    close_ledger();
    return fmt("rc %d", rc);
  }};
}
// a witness of the wrong shape is refused before anything runs, at each of the four doors
Scenario wrong_shape(const char *name, int door) {
  return Scenario{name, false, [=](bool) {
    World w(2, N_AUX, 13, 2);
    w.views[1].n_aux--;
    groth16::Proof proofs[2];
    int codes[2];
    return ledgered(w, [&] {
      if (door == 0) groth16::prove_witness(*w.shape, *w.params, w.inputs.data(), 2, w.aux.data(), N_AUX - 1, w.r[0], w.s[0]);
      if (door == 1) groth16::prove_witness_part(*w.shape, *w.params, w.inputs.data(), 2, w.aux.data(), N_AUX - 1, 0, 1);
      if (door == 2) groth16::prove_witness_batch_codes(*w.shape, *w.params, w.views.data(), 2, w.r.data(), w.s.data(), proofs, codes);
      if (door == 3) w.shape->which_is_unsatisfied(w.views.data(), 2);
      return std::string();
    });
  }};
}

// prove_witness_batch_dev_codes over World's resident witnesses (n_in inputs, N_AUX aux, 13 constraints)
Scenario dev_batch(const char *name, size_t n_in, size_t k, size_t pad, unsigned flags, int mode, size_t budget, bool sweep) {
  return Scenario{name, sweep, [=](bool idd) {
    World w(n_in, N_AUX, 13, k, 0, idd);
    const groth16::DeviceWitnesses dw = w.resident(pad);
    const bool checked = flags & BH_PROVE_CHECK;
    if (checked) check_answers = {BH_R1CS_SATISFIED, BH_R1CS_SATISFIED, 7, BH_R1CS_SATISFIED};
    std::vector<groth16::Proof> proofs(k);
    std::vector<int> codes(k, -99);
    std::vector<uint32_t> bad(k, 0);
    return ledgered(w, [&] {
      groth16::prove_witness_batch_dev_codes(*w.shape, *w.params, dw, w.r.data(), w.s.data(), flags, nullptr, proofs.data(), codes.data(),
                                             checked ? bad.data() : nullptr, nullptr, budget, mode);
      std::string t = codes_text(codes);
      if (checked) { t += " first_unsatisfied"; for (uint32_t x : bad) t += fmt(" %u", x); }
      return t;
    });
  }};
}
// what prove_witness_batch_dev_codes refuses before anything runs, and k = 0
Scenario dev_refusals(const char *name) {
  return Scenario{name, false, [=](bool) {
    World w(2, N_AUX, 13, 2);
    const groth16::DeviceWitnesses ok = w.resident(0);
    groth16::Proof proofs[2];
    int codes[2];
    std::string t;
    auto attempt = [&](const char *what, groth16::DeviceWitnesses dw, unsigned flags, int mode) {
      t += fmt(" [%s: ", what) + outcome_of([&] {
        groth16::prove_witness_batch_dev_codes(*w.shape, *w.params, dw, w.r.data(), w.s.data(), flags, nullptr, proofs, codes, nullptr,
                                               nullptr, 0, mode);
        return std::string();
      }) + "]";
    };
    groth16::DeviceWitnesses dw = ok;
    dw.in_stride += 8;
    attempt("stride no multiple of 32", dw, 0, groth16::BATCH_AUTO);
    dw = ok;
    dw.aux_stride -= 32;
    attempt("stride shorter than the vector", dw, 0, groth16::BATCH_AUTO);
    attempt("both finish bits", ok, BH_PROVE_FINISH_DEVICE | BH_PROVE_FINISH_HOST, groth16::BATCH_AUTO);
    attempt("unknown flag", ok, 8u, groth16::BATCH_AUTO);
    attempt("mode BATCH_GROUPED", ok, 0, groth16::BATCH_GROUPED);
    dw = ok;
    dw.inputs = nullptr;
    attempt("null buffer", dw, 0, groth16::BATCH_AUTO);
    dw = ok;
    dw.k = 0;
    attempt("k = 0", dw, 0, groth16::BATCH_AUTO);
    close_ledger();
    return "refusals" + t;
  }};
}

std::vector<Scenario> scenarios() {
  std::vector<Scenario> v;
  // the `inputs` multiexps go to the host at <= 8 terms; the two issue strategies split at log_m <= 16
  v.push_back(single("single proof, host-evaluated, 2 inputs, domain 2^4", true, 2, 13));
  v.push_back(single("single proof, device-evaluated, 2 inputs, domain 2^4", false, 2, 13));
  v.push_back(single("single proof, host-evaluated, 9 inputs, domain 2^4", true, 9, 13));
  v.push_back(single("single proof, device-evaluated, 9 inputs, domain 2^4", false, 9, 13));
  v.push_back(single("single proof, host-evaluated, 2 inputs, domain 2^17", true, 2, 65537));
  v.push_back(single("single proof, device-evaluated, 9 inputs, domain 2^17", false, 9, 65537));
  v.push_back(Scenario{"prove_witness_part 1 of 3 (base offsets by popcount)", true, [](bool idd) {
    World w(2, N_AUX, 300, 1, 0, idd);
    return ledgered(w, [&] {
      groth16::prove_witness_part(*w.shape, *w.params, w.inputs.data(), 2, w.aux.data(), N_AUX, 1, 3);
      return std::string();
    });
  }});
  v.push_back(batch("batch BATCH_AUTO k=3", groth16::BATCH_AUTO, 3, 0, 0, false, false));
  // m = 16: a coefficient vector is 512 bytes.  BATCH_GROUPED: g + 3 vectors in the budget; the batched modes: 4 g
  v.push_back(batch("batch BATCH_GROUPED k=5 in groups of 2, 2, 1", groth16::BATCH_GROUPED, 5, 5 * 512, 0, false, true));
  v.push_back(batch("batch BATCH_GROUPED_H k=5 in groups of 2, 2, 1", groth16::BATCH_GROUPED_H, 5, 8 * 512, 0, false, true));
  v.push_back(batch("batch BATCH_GROUPED_HE k=5 in groups of 2, 2, 1, adjacent host vectors", groth16::BATCH_GROUPED_HE, 5, 8 * 512, 0, false, true));
  v.push_back(batch("batch BATCH_GROUPED_HE k=5 in groups of 2, 2, 1, host vectors apart", groth16::BATCH_GROUPED_HE, 5, 8 * 512, 3, false, true));
  v.push_back(batch("checked batch BATCH_AUTO k=4, witness 2 unsatisfied", groth16::BATCH_AUTO, 4, 0, 0, true, false));
  v.push_back(batch("checked batch BATCH_GROUPED k=4 (one group), witness 2 unsatisfied", groth16::BATCH_GROUPED, 4, 0, 0, true, true));
  v.push_back(call_sites("call sites mode 0", 0));
  v.push_back(call_sites("call sites mode 1", 1));
  v.push_back(call_sites("call sites mode 2", 2));
  v.push_back(wrong_shape("wrong-shaped witness: prove_witness", 0));
  v.push_back(wrong_shape("wrong-shaped witness: prove_witness_part", 1));
  v.push_back(wrong_shape("wrong-shaped witness: prove_witness_batch_codes", 2));
  v.push_back(wrong_shape("wrong-shaped witness: which_is_unsatisfied", 3));
  // ---- the second part of the record: witnesses in device memory (prove_witness_batch_dev_codes).  Domain 16 as above
  const unsigned CHECK = BH_PROVE_CHECK, ON_DEV = BH_PROVE_FINISH_DEVICE, ON_HOST = BH_PROVE_FINISH_HOST;
  v.push_back(dev_batch("dev in-flight, one witness", 2, 1, 0, 0, groth16::BATCH_AUTO, 0, true));
  v.push_back(dev_batch("dev in-flight, inputs on device", 9, 1, 0, ON_HOST, groth16::BATCH_AUTO, 0, true));
  v.push_back(dev_batch("dev in-flight k=3", 2, 3, 96, 0, groth16::BATCH_AUTO, 0, false));
  v.push_back(dev_batch("dev grouped k=5 in groups of 2, 2, 1", 2, 5, 0, ON_HOST, groth16::BATCH_GROUPED_HE, 8 * 512, true));
  // (a group cap of 3: the groups {0, 1} and {3, 4} show the break at the unsatisfied witness, not the cap)
  v.push_back(dev_batch("dev grouped, checked, witness 2 unsatisfied", 2, 5, 96, CHECK | ON_DEV, groth16::BATCH_GROUPED_HE, 12 * 512, true));
  v.push_back(dev_batch("dev grouped, inputs on device", 9, 3, 96, ON_HOST, groth16::BATCH_GROUPED_HE, 0, true));
  v.push_back(dev_batch("dev in-flight, checked, witness 2 unsatisfied", 2, 4, 0, CHECK, groth16::BATCH_AUTO, 0, false));
  v.push_back(dev_refusals("dev refusals"));
  return v;
}
}  // namespace

int main(int argc, char **argv) {
  const bool record = argc == 3 && !strcmp(argv[1], "--record");
  if (argc != 2 && !record) {
    fprintf(stderr, "usage: %s EXPECTED | --record FILE\n", argv[0]);
    return 2;
  }
  std::ostringstream out;
  for (const Scenario &sc : scenarios()) play(sc, out);
  const std::string got = out.str();
  for (const std::string &d : dirty) fprintf(stderr, "prover_calls: ledger: %s\n", d.c_str());
  if (record) {   // (the record holds calls and outcomes; a dirty ledger of the recorded code is reported, not recorded)
    std::ofstream(argv[2]) << got;
    printf("prover_calls: recorded %zu bytes\n", got.size());
    return 0;
  }
  std::ifstream f(argv[1]);
  std::stringstream want;
  want << f.rdbuf();
  if (!f || want.str() != got) {
    std::istringstream a(want.str()), b(got);
    std::string la, lb;
    for (size_t n = 1;; n++) {
      const bool ha = (bool)std::getline(a, la), hb = (bool)std::getline(b, lb);
      if (!ha && !hb) break;
      if (ha != hb || la != lb) {
        fprintf(stderr, "prover_calls: line %zu differs\n  expected: %s\n  got:      %s\n", n, ha ? la.c_str() : "<end>", hb ? lb.c_str() : "<end>");
        break;
      }
    }
    return 1;
  }
  if (!dirty.empty()) {
    fprintf(stderr, "prover_calls: %zu runs left the ledger dirty\n", dirty.size());
    return 1;
  }
  printf("prover_calls: %zu bytes of transcript and unwind outcomes match, every ledger clean\n", got.size());
  return 0;
}
