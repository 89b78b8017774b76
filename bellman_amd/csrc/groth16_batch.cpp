// k proofs of one circuit in one call: prove_witness_batch (host witnesses) and prove_witness_batch_dev (witnesses in device
// memory), their checked / codes forms and the C tails.  The single proof they are built on is groth16_prover.cpp.
#include <string.h>

#include <algorithm>
#include <array>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "groth16_internal.hpp"

namespace groth16 {
using namespace bellman;
using namespace detail;

// ---- the grouped path ---------------------------------------------------------------------------------------------------
// Across the proofs of one circuit the bases and the density maps are the same; only the scalar vectors differ.  So the
// five long multiexps of every proof (l, a_aux, b_g1_aux, b_g2_aux, h) are issued as five many-jobs over all the witnesses
// of a group (bh_msm_many_async_dev: one launch chain for the group where the library's size rule takes the many-plan, k
// ordinary jobs otherwise), the h blocks run on one stream into strided coefficient vectors, and the `inputs` multiexps and
// finish_proof stay per witness.  Both entries cut groups by one rule and run them through one body, group_sums.

// A group is a run of consecutive indices good[first ..) of at most `cap` witnesses: its vectors then lie one stride apart
// behind its first witness'.  (Host witnesses are uploaded group by group: there `good` is 0 .. k-1 and a group `cap` long.)
static size_t run_length(const std::vector<size_t> &good, size_t first, size_t cap) {
  size_t g = 1;
  while (first + g < good.size() && g < cap && good[first + g] == good[first + g - 1] + 1) g++;
  return g;
}
// The most witnesses in a group: within the budget (0: the default) the group holds, of coefficient vectors of `vec` bytes,
// BATCH_GROUPED: one per witness (the a vector of its h block, which becomes its quotient) plus the b and c vectors and the
// FFT scratch, which the h blocks of a group share (they run one after the other on one stream);
// BATCH_GROUPED_H / _HE: a, b, c and a scratch vector per witness (ONE batched h block).
static size_t group_cap(int mode, size_t workspace_budget, size_t vec) {
  const size_t vecs = (workspace_budget ? workspace_budget : BATCH_WORKSPACE_BYTES) / vec;
  return std::min<size_t>(std::max<size_t>(mode == BATCH_GROUPED ? (vecs > 3 ? vecs - 3 : 1) : vecs / 4, 1), 4096);
}

// The sums and per-slot codes of one group: the w.k witnesses whose vectors lie in device memory at w (the caller's buffers,
// or this call's uploads: `upload` - if any - queues them on the group's stream before the first many-job).  host_inputs:
// per witness its host input vector where the `inputs` multiexps are answered on the host, null where they run on the
// device.  mode: BATCH_GROUPED, _H (every witness has its own a, b, c and scratch vector - its h blocks run as ONE batched h
// block) or _HE (the same, and the group's constraint evaluations run as ONE bh_r1cs_eval_many_dev).  A runtime failure
// throws once the group's jobs have drained.
static void group_sums(const R1cs &r1cs, Parameters &params, const Densities &dens, const QueryTable &queries_of, int mode,
                       const DeviceWitnesses &w, const Fr *const *host_inputs, const std::function<void(void *stream)> &upload,
                       MsmSums *sums, std::array<int, N_SLOTS> *rcs, double &h_ms, double &msm_ms) {
  bh_ctx *ctx = params.ctx;
  const size_t g = w.k, n_in = r1cs.num_inputs, n_aux = r1cs.num_aux;
  const Domain dom = domain_of(r1cs.num_constraints);
  const size_t m = dom.m, vec = m * 32;
  const uint32_t log_m = dom.log_m;
  const bool many_eval = mode == BATCH_GROUPED_HE, batched_h = mode == BATCH_GROUPED_H || many_eval;
  const char *d_in = (const char *)w.inputs, *d_aux = (const char *)w.aux;
  const double t1 = now_ms();
  const size_t bc_vecs = batched_h ? g : 1, scratch_bytes = log_m > 11 ? bc_vecs * vec : 32;
  DevBuf da(ctx, g * vec), db(ctx, bc_vecs * vec), dc(ctx, bc_vecs * vec), dscratch(ctx, scratch_bytes);
  ProofStream ps(ctx);
  StreamDrain drain{ps};
  InFlight<bh_msm_job> in_jobs(g * N_SLOTS);   // witness j's `inputs` multiexps at j * N_SLOTS + slot
  InFlight<bh_msm_many_job> many_jobs(N_SLOTS);
  // 1. the witnesses, where they are not resident
  if (upload) upload(ps.st);
  // 2. the many-jobs over the aux vectors and the shared bases and densities, ordered after the uploads
  auto issue_many = [&](Slot slot, const void *scalars, size_t stride, size_t n) {
    const Query &q = queries_of[slot];
    const uint64_t *d = dens.dev_of(q.density);
    check(bh_msm_many_async_dev(ctx, q.bases, q.skip, scalars, stride, n, g, BH_SCALARS_MONT, d, d ? n : 0, nullptr, ps.st,
                                &many_jobs.at[slot]));
  };
  for (Slot slot : ISSUE_ORDER)
    if (queries_of[slot].scalars == FROM_AUX) issue_many(slot, d_aux, w.aux_stride, n_aux);
  // 3. the h block per witness, on one stream, into the group's strided coefficient vectors; then the H many-job,
  // ordered after them
  if (many_eval)
    check(bh_r1cs_eval_many_dev(ctx, r1cs.handle, d_in, w.in_stride, d_aux, w.aux_stride, g, da.p, db.p, dc.p, vec, log_m, ps.st));
  for (size_t j = 0; j < g && !many_eval; j++) {
    void *a_j = (char *)da.p + j * vec;
    const size_t bc = batched_h ? j * vec : 0;
    check(bh_r1cs_eval_dev(ctx, r1cs.handle, d_in + j * w.in_stride, d_aux + j * w.aux_stride, a_j, (char *)db.p + bc,
                           (char *)dc.p + bc, log_m, ps.st));
    if (!batched_h) check(bh_h_poly_fr_dev_on(ctx, a_j, db.p, dc.p, dscratch.p, log_m, ps.st));
  }
  if (batched_h)
    check(bh_h_poly_fr_many_dev_on(ctx, da.p, db.p, dc.p, vec, g, log_m, BH_FFT_MANY_FORCE, dscratch.p, scratch_bytes, ps.st));
  issue_many(H, da.p, vec, m - 1);   // a.len() - 1
  // 4. the `inputs` multiexps as the single call issues them (a handful of terms: answered on the host, at issue time -
  // so they come last, while the GPU works)
  for (size_t j = 0; j < g; j++)
    for (Slot slot : ISSUE_ORDER) {
      const Query &q = queries_of[slot];
      if (q.scalars != FROM_INPUTS) continue;
      const uint64_t *dh = dens.host_of(q.density), *dd = dens.dev_of(q.density);
      bh_msm_job **job = &in_jobs.at[j * N_SLOTS + slot];
      if (host_inputs)
        check(bh_msm_async(ctx, q.bases, q.skip, host_inputs[j], n_in, BH_SCALARS_MONT, dh, dh ? n_in : 0, job));
      else
        check(bh_msm_async_dev_after(ctx, q.bases, q.skip, d_in + j * w.in_stride, n_in, BH_SCALARS_MONT, dd, dd ? n_in : 0, nullptr,
                                     ps.st, job));
    }
  const double t2 = now_ms();
  // waits, every job even when an earlier one fails; codes per proof by slot (prover.rs:339-354): each witness' `inputs`
  // jobs, then the many-jobs, both in wait order
  for (size_t j = 0; j < g; j++)
    for (Slot slot : WAIT_ORDER)
      if (queries_of[slot].scalars == FROM_INPUTS) rcs[j][slot] = bh_msm_wait(in_jobs.take(j * N_SLOTS + slot), sum_at(sums[j], slot));
  std::vector<unsigned char> recs(g * sizeof(G2Affine));
  std::vector<int32_t> codes_v(g);
  for (Slot slot : WAIT_ORDER) {
    if (queries_of[slot].scalars == FROM_INPUTS) continue;
    check(bh_msm_many_wait(many_jobs.take(slot), recs.data(), codes_v.data(), nullptr, nullptr));
    for (size_t j = 0; j < g; j++) {
      memcpy(sum_at(sums[j], slot), recs.data() + j * slot_bytes(slot), slot_bytes(slot));
      rcs[j][slot] = codes_v[j];
    }
  }
  h_ms += t2 - t1;
  msm_ms += now_ms() - t2;
}

// ---- k proofs from host witnesses ------------------------------------------------------------------------------------------
// Error order per proof: prove_core's.
void prove_witness_batch_codes(const R1cs &r1cs, Parameters &params, const WitnessView *witnesses, size_t k, const Fr *r, const Fr *s,
                               Proof *proofs, int *codes, ProveTimings *tm, size_t workspace_budget, int mode) {
  require_shape(r1cs, witnesses, k);
  if (tm) *tm = ProveTimings{0, 0, 0, 0};
  if (!k) return;
  const double t0 = now_ms();
  // BATCH_AUTO never takes the grouped path (many-jobs over a group of witnesses) by itself.  Measured
  // (tools/bench_prove_batch.py, profiles/prove_batch_bench.json: MiMC-322 and the chain circuit at 2^14 / 2^16 / 2^18
  // constraints, k = 4 and 16): against k prove_witness_async calls in flight it is 0.51 - 0.66 x on MiMC-322 and
  // 0.97 - 1.29 x on the chain circuit, beyond the baseline's own spread at two shapes of eight (k = 16 at 2^16 and 2^18) -
  // and at another one (2^16, k = 4) in the run before.  No basis for a rule yet.
  if (mode != BATCH_GROUPED && mode != BATCH_GROUPED_H && mode != BATCH_GROUPED_HE) {
    // k proofs by the single-proof path, BATCH_IN_FLIGHT of them in flight (device memory stays bounded), waited in order
    std::vector<std::unique_ptr<AsyncProof>> jobs(k);
    auto finish = [&](size_t j) {
      ProveTimings one = {0, 0, 0, 0};
      try {
        proofs[j] = jobs[j]->wait(&one);
        codes[j] = BH_OK;
      } catch (const SynthesisError &e) {
        if (e.code < 0) { jobs.clear(); throw; }   // (the remaining jobs join in their destructors)
        codes[j] = e.code;
      }
      jobs[j].reset();
      if (tm) { tm->h_poly_ms += one.h_poly_ms; tm->msm_ms += one.msm_ms; }
    };
    for (size_t j = 0; j < k; j++) {
      if (j >= BATCH_IN_FLIGHT) finish(j - BATCH_IN_FLIGHT);
      jobs[j] = prove_witness_async(r1cs, params, witnesses[j].inputs, witnesses[j].n_inputs, witnesses[j].aux, witnesses[j].n_aux,
                                    r[j], s[j]);
    }
    for (size_t j = k > BATCH_IN_FLIGHT ? k - BATCH_IN_FLIGHT : 0; j < k; j++) finish(j);
    if (tm) tm->total_ms = (float)(now_ms() - t0);
    return;
  }
  bh_ctx *ctx = params.ctx;
  const size_t in_stride = r1cs.num_inputs * 32, aux_stride = r1cs.num_aux * 32;
  const size_t cap = std::min(k, group_cap(mode, workspace_budget, domain_of(r1cs.num_constraints).m * 32));
  Blinding blind(params, r, s, k);   // beside the GPU work
  Densities dens;
  dens.of(r1cs);
  const QueryTable queries_of = queries(params, r1cs.num_inputs, dens.b_in_total);
  std::vector<size_t> all(k);
  std::vector<const Fr *> host_inputs;
  for (size_t j = 0; j < k; j++) {
    all[j] = j;
    if (r1cs.num_inputs <= HOST_INPUTS_MAX) host_inputs.push_back(witnesses[j].inputs);
  }
  std::vector<MsmSums> sums(k);
  std::vector<std::array<int, N_SLOTS>> rcs(k);
  double h_ms = 0, msm_ms = 0;
  for (size_t first = 0, g; first < k; first += g) {
    g = run_length(all, first, cap);
    // one strided buffer per vector kind (BATCH_GROUPED_HE: in one upload each where the host vectors are adjacent); their
    // allocation counts with the h block, as the body's own buffers do
    const double t1 = now_ms();
    DevBuf d_in(ctx, g * in_stride + 32), d_aux(ctx, g * aux_stride + 32);
    h_ms += now_ms() - t1;
    group_sums(r1cs, params, dens, queries_of, mode, DeviceWitnesses{d_in.p, in_stride, d_aux.p, aux_stride, g},
               host_inputs.empty() ? nullptr : &host_inputs[first],
               [&](void *st) { upload_witnesses(ctx, witnesses + first, g, d_in.p, d_aux.p, st, mode == BATCH_GROUPED_HE); },
               &sums[first], &rcs[first], h_ms, msm_ms);
  }
  blind.join();
  if (blind.error && !subverted(params)) std::rethrow_exception(blind.error);
  for (size_t j = 0; j < k; j++) {
    const int code = first_failure(params, rcs[j].data());
    if (code < 0) check(code);   // a runtime failure is the call's
    codes[j] = code;
    if (code == BH_OK) proofs[j] = finish_proof(blind.terms[j], sums[j], r[j], s[j]);
  }
  if (tm) {
    tm->h_poly_ms = (float)h_ms;
    tm->msm_ms = (float)msm_ms;
    tm->total_ms = (float)(now_ms() - t0);
  }
}

// first_bad[0 .. k) of a check into the indices of the satisfied witnesses; the others get BH_ERR_UNSATISFIABLE
static std::vector<size_t> satisfied(const std::vector<uint32_t> &first_bad, int *codes, uint32_t *first_unsatisfied) {
  std::vector<size_t> good;
  for (size_t j = 0; j < first_bad.size(); j++) {
    if (first_unsatisfied) first_unsatisfied[j] = first_bad[j];
    if (first_bad[j] == BH_R1CS_SATISFIED) good.push_back(j);
    else codes[j] = BH_ERR_UNSATISFIABLE;
  }
  return good;
}

void prove_witness_batch_checked_codes(const R1cs &r1cs, Parameters &params, const WitnessView *witnesses, size_t k, const Fr *r,
                                       const Fr *s, Proof *proofs, int *codes, uint32_t *first_unsatisfied, ProveTimings *tm,
                                       size_t workspace_budget, int mode) {
  if (tm) *tm = ProveTimings{0, 0, 0, 0};
  const double t0 = now_ms();
  const std::vector<uint32_t> first_bad =
      check_witnesses(params.ctx, r1cs, witnesses, k, workspace_budget ? workspace_budget : BATCH_WORKSPACE_BYTES);
  const double pre_ms = now_ms() - t0;
  // the satisfied witnesses, in order, through the unchecked batch
  const std::vector<size_t> good = satisfied(first_bad, codes, first_unsatisfied);
  const size_t n = good.size();
  std::vector<WitnessView> ws(n);
  std::vector<Fr> rr(n), ss(n);
  std::vector<Proof> ps(n);
  std::vector<int> cs(n, BH_OK);
  for (size_t i = 0; i < n; i++) { ws[i] = witnesses[good[i]]; rr[i] = r[good[i]]; ss[i] = s[good[i]]; }
  prove_witness_batch_codes(r1cs, params, ws.data(), n, rr.data(), ss.data(), ps.data(), cs.data(), tm, workspace_budget, mode);
  for (size_t i = 0; i < n; i++) { proofs[good[i]] = ps[i]; codes[good[i]] = cs[i]; }
  if (tm) { tm->synthesis_ms = (float)pre_ms; tm->total_ms = (float)(now_ms() - t0); }
}

// ---- k proofs from witnesses that are in device memory already (groth16.hpp DeviceWitnesses) ---------------------------
// The finish rule of flags without a finish bit: device finishing where it was measured ahead of host finishing by more
// than the host variant's own spread at every shape of that k.  Measured (tools/bench_prove_batch_dev.py,
// profiles/prove_batch_dev_bench.json, DESIGN.md 5.5.2: MiMC-322, chain 2^14 / 2^16, boolean 2^16; k = 16 and 256): ahead at
// three of the four k = 256 shapes in each of three runs, at chain 2^16 x 256 in one run of three, and at no k = 16 shape -
// no k qualifies reproducibly: never.  Device finishing is forced-only, as the grouped path is (mode 3 over device
// witnesses: 0.54 - 0.90 x the proofs in flight at k = 256, same file).
static bool finish_on_device_by_rule(size_t /*k*/, size_t /*n_constraints*/) { return false; }

void prove_witness_batch_dev_codes(const R1cs &r1cs, Parameters &params, const DeviceWitnesses &w, const Fr *r, const Fr *s,
                                   unsigned flags, void *stream, Proof *proofs, int *codes, uint32_t *first_unsatisfied,
                                   ProveTimings *tm, size_t workspace_budget, int mode) {
  const size_t k = w.k, n_in = r1cs.num_inputs, n_aux = r1cs.num_aux;
  if (mode != BATCH_AUTO && mode != BATCH_GROUPED_HE) throw std::invalid_argument("mode: BATCH_AUTO or BATCH_GROUPED_HE");
  if ((flags & BH_PROVE_FINISH_DEVICE) && (flags & BH_PROVE_FINISH_HOST)) throw std::invalid_argument("both finish bits");
  if (flags & ~(BH_PROVE_CHECK | BH_PROVE_FINISH_DEVICE | BH_PROVE_FINISH_HOST)) throw std::invalid_argument("unknown flag");
  // the layout rules of bh_r1cs_check_many_dev, before anything runs
  if (w.in_stride % 32 || w.aux_stride % 32 || w.in_stride < n_in * 32 || w.aux_stride < n_aux * 32)
    throw std::invalid_argument("witness strides: multiples of 32 bytes, at least the vector's length");
  if (k && ((n_in && !w.inputs) || (n_aux && !w.aux))) throw std::invalid_argument("null witness buffer");
  if (tm) *tm = ProveTimings{0, 0, 0, 0};
  if (!k) return;
  bh_ctx *ctx = params.ctx;
  const double t0 = now_ms();
  // whatever wrote the witnesses (the caller's solve) has finished; null is the context's stream
  check(bh_stream_synchronize(ctx, stream));
  auto in_at = [&](size_t j) { return (const char *)w.inputs + j * w.in_stride; };
  auto aux_at = [&](size_t j) { return (const char *)w.aux + j * w.aux_stride; };

  // which witnesses are proved: all of them, or the satisfied ones - by index, nothing is copied or compacted
  std::vector<uint32_t> first_bad(k, BH_R1CS_SATISFIED);
  if (flags & BH_PROVE_CHECK) {
    DevBuf d_bad(ctx, k * sizeof(uint32_t));
    ProofStream ps(ctx);
    StreamDrain drain{ps};
    check(bh_r1cs_check_many_dev(ctx, r1cs.handle, w.inputs, w.in_stride, w.aux, w.aux_stride, k, (uint32_t *)d_bad.p, ps.st));
    check(bh_stream_synchronize(ctx, ps.st));
    check(bh_dev_download(ctx, first_bad.data(), d_bad.p, k * sizeof(uint32_t)));
  }
  const std::vector<size_t> good = satisfied(first_bad, codes, (flags & BH_PROVE_CHECK) ? first_unsatisfied : nullptr);
  const double t1 = now_ms();
  const size_t n = good.size();
  // the `inputs` multiexps of a few terms are answered on the host: one small download of the input vectors
  std::vector<Fr> h_in;
  if (n_in && n_in <= HOST_INPUTS_MAX) {
    h_in.resize(k * n_in);
    if (w.in_stride == n_in * 32) check(bh_dev_download(ctx, h_in.data(), w.inputs, k * n_in * 32));
    else
      for (size_t j = 0; j < k; j++) check(bh_dev_download(ctx, h_in.data() + j * n_in, in_at(j), n_in * 32));
  }
  std::vector<const Fr *> host_inputs;   // of the proved witnesses; empty: the `inputs` multiexps run on the device
  for (size_t i = 0; i < n && !h_in.empty(); i++) host_inputs.push_back(h_in.data() + good[i] * n_in);
  const bool on_device = (flags & BH_PROVE_FINISH_DEVICE) ||
                         (!(flags & BH_PROVE_FINISH_HOST) && finish_on_device_by_rule(k, r1cs.num_constraints));
  std::vector<Fr> rr(n), ss(n);
  for (size_t i = 0; i < n; i++) { rr[i] = r[good[i]]; ss[i] = s[good[i]]; }
  // (host finishing: the blinding terms beside the GPU work, as in every other path; an identity delta fails there)
  std::unique_ptr<Blinding> blind;
  if (!on_device && n) blind.reset(new Blinding(params, rr.data(), ss.data(), n));

  // the eight multiexps of every proved witness by the single-proof path, BATCH_IN_FLIGHT at a time, waited in order
  // (BATCH_GROUPED_HE, forced only: by the grouped path - a group's vectors are the caller's pointers at its first witness
  // with the caller's strides, so an unsatisfied witness in between ends a group: nothing is copied)
  struct Job {
    std::thread th;
    MsmSums sums;
    ProveTimings tm = {0, 0, 0, 0};
    std::exception_ptr error;
    ~Job() { if (th.joinable()) th.join(); }   // whatever unwinds this frame: the job is drained first
  };
  std::vector<MsmSums> sums(n);
  std::vector<int> rc(n, BH_OK);
  std::exception_ptr fatal;
  double h_ms = 0, msm_ms = 0;
  if (mode == BATCH_GROUPED_HE) {
    try {
      const size_t cap = group_cap(mode, workspace_budget, domain_of(r1cs.num_constraints).m * 32);
      Densities dens;
      dens.of(r1cs);
      const QueryTable queries_of = queries(params, n_in, dens.b_in_total);
      std::vector<std::array<int, N_SLOTS>> rcs(n);
      for (size_t first = 0, g; first < n; first += g) {
        g = run_length(good, first, cap);
        group_sums(r1cs, params, dens, queries_of, mode,
                   DeviceWitnesses{in_at(good[first]), w.in_stride, aux_at(good[first]), w.aux_stride, g},
                   host_inputs.empty() ? nullptr : &host_inputs[first], nullptr, &sums[first], &rcs[first], h_ms, msm_ms);
      }
      // a proof's code: the first failing wait's (prover.rs:339-354); a runtime failure is the call's
      for (size_t i = 0; i < n; i++) {
        for (Slot slot : WAIT_ORDER)
          if (rcs[i][slot] != BH_OK) { rc[i] = rcs[i][slot]; break; }
        if (rc[i] < 0) check(rc[i]);
      }
    } catch (...) {
      fatal = std::current_exception();   // (its jobs have drained: InFlight)
    }
  }
  std::vector<std::unique_ptr<Job>> jobs(n);   // declared after everything a job writes: destroyed, and so joined, first
  auto finish = [&](size_t i) {
    Job &job = *jobs[i];
    job.th.join();
    if (job.error) {
      try {
        std::rethrow_exception(job.error);
      } catch (const SynthesisError &e) {
        if (e.code < 0) { if (!fatal) fatal = job.error; }
        else rc[i] = e.code;
      } catch (...) {
        if (!fatal) fatal = job.error;
      }
    }
    sums[i] = job.sums;
    h_ms += job.tm.h_poly_ms;
    msm_ms += job.tm.msm_ms;
    jobs[i].reset();
  };
  for (size_t i = 0; i < n && mode == BATCH_AUTO; i++) {
    if (i >= BATCH_IN_FLIGHT) finish(i - BATCH_IN_FLIGHT);
    AssignmentSource src;
    src.n_in = n_in; src.n_aux = n_aux; src.n_cons = r1cs.num_constraints; src.r1cs = &r1cs;
    src.inputs = host_inputs.empty() ? nullptr : host_inputs[i];
    src.aux = nullptr;
    src.resident = true;
    src.inputs_dev = in_at(good[i]);
    src.aux_dev = aux_at(good[i]);
    jobs[i].reset(new Job());
    Job *job = jobs[i].get();
    Parameters *pp = &params;
    job->th = std::thread([job, src, pp] {
      try { msm_sums(src, *pp, 0, 1, job->sums, &job->tm); } catch (...) { job->error = std::current_exception(); }
    });
  }
  for (size_t i = n > BATCH_IN_FLIGHT ? n - BATCH_IN_FLIGHT : 0; i < n && mode == BATCH_AUTO; i++) finish(i);   // all drained
  if (blind) blind->join();
  if (fatal) std::rethrow_exception(fatal);
  if (blind && blind->error && !subverted(params)) std::rethrow_exception(blind->error);
  // an identity delta beats whatever a multiexp reported (first_failure, groth16_internal.hpp)
  for (size_t i = 0; i < n; i++) codes[good[i]] = subverted(params) ? BH_ERR_UNEXPECTED_IDENTITY : rc[i];
  if (!subverted(params)) {
    if (on_device) {
      // the sums of the proofs that have them, k' x 960 on the host, uploaded once; the proofs come back in one download
      std::vector<size_t> done;
      for (size_t i = 0; i < n; i++)
        if (rc[i] == BH_OK) done.push_back(i);
      std::vector<MsmSums> m(done.size());
      std::vector<Fr> r2(done.size()), s2(done.size());
      for (size_t d = 0; d < done.size(); d++) { m[d] = sums[done[d]]; r2[d] = rr[done[d]]; s2[d] = ss[done[d]]; }
      const std::vector<Proof> out = assemble_proofs(params, m.data(), r2.data(), s2.data(), done.size());
      for (size_t d = 0; d < done.size(); d++) proofs[good[done[d]]] = out[d];
    } else {
      for (size_t i = 0; i < n; i++)
        if (rc[i] == BH_OK) proofs[good[i]] = finish_proof(blind->terms[i], sums[i], rr[i], ss[i]);
    }
  }
  if (tm) {
    tm->synthesis_ms = (float)(t1 - t0);
    tm->h_poly_ms = (float)h_ms;
    tm->msm_ms = (float)msm_ms;
    tm->total_ms = (float)(now_ms() - t0);
  }
}

// ---- the forms that return vectors and throw ------------------------------------------------------------------------------
namespace {
// k proofs, their codes and the first unsatisfied constraints, with r and s split out of the pairs
struct BatchResult {
  std::vector<Fr> r, s;
  std::vector<Proof> proofs;
  std::vector<int> codes;
  std::vector<uint32_t> first_bad;
  BatchResult(const std::vector<std::pair<Fr, Fr>> &rs, size_t k) : r(k), s(k), proofs(k), codes(k, BH_OK), first_bad(k, BH_R1CS_SATISFIED) {
    if (k != rs.size()) throw std::invalid_argument("one (r, s) per witness");
    for (size_t j = 0; j < k; j++) { r[j] = rs[j].first; s[j] = rs[j].second; }
  }
  std::vector<Proof> take() {   // throws what the first failing proof would throw
    for (int code : codes) check(code);
    return std::move(proofs);
  }
};
}  // namespace

std::vector<Proof> prove_witness_batch(const R1cs &r1cs, Parameters &params, const std::vector<WitnessView> &witnesses,
                                       const std::vector<std::pair<Fr, Fr>> &rs, ProveTimings *tm, size_t workspace_budget, int mode) {
  BatchResult b(rs, witnesses.size());
  prove_witness_batch_codes(r1cs, params, witnesses.data(), witnesses.size(), b.r.data(), b.s.data(), b.proofs.data(), b.codes.data(),
                            tm, workspace_budget, mode);
  return b.take();
}

std::vector<Proof> prove_witness_batch_checked(const R1cs &r1cs, Parameters &params, const std::vector<WitnessView> &witnesses,
                                               const std::vector<std::pair<Fr, Fr>> &rs, std::vector<uint32_t> *first_unsatisfied,
                                               ProveTimings *tm, size_t workspace_budget, int mode) {
  BatchResult b(rs, witnesses.size());
  prove_witness_batch_checked_codes(r1cs, params, witnesses.data(), witnesses.size(), b.r.data(), b.s.data(), b.proofs.data(),
                                    b.codes.data(), b.first_bad.data(), tm, workspace_budget, mode);
  if (first_unsatisfied) *first_unsatisfied = b.first_bad;
  return b.take();
}

std::vector<Proof> prove_witness_batch_dev(const R1cs &r1cs, Parameters &params, const DeviceWitnesses &w,
                                           const std::vector<std::pair<Fr, Fr>> &rs, unsigned flags, void *stream,
                                           std::vector<uint32_t> *first_unsatisfied, ProveTimings *tm) {
  BatchResult b(rs, w.k);
  prove_witness_batch_dev_codes(r1cs, params, w, b.r.data(), b.s.data(), flags, stream, b.proofs.data(), b.codes.data(),
                                (flags & BH_PROVE_CHECK) ? b.first_bad.data() : nullptr, tm);
  if (first_unsatisfied && (flags & BH_PROVE_CHECK)) *first_unsatisfied = b.first_bad;
  return b.take();
}

}  // namespace groth16

// ---- the C tails ------------------------------------------------------------------------------------------------------------
// rcs[j], and proof j's 384 bytes or zeros
static void write_results(const std::vector<groth16::Proof> &proofs, const std::vector<int> &codes, void *proofs_out, int32_t *rcs) {
  for (size_t j = 0; j < codes.size(); j++) {
    char *out = (char *)proofs_out + j * 384;
    rcs[j] = codes[j];
    if (codes[j] == BH_OK) write_proof(out, proofs[j]);
    else memset(out, 0, 384);
  }
}

// bh_groth16_prove_witness_batch_dev
int prove_witness_batch_dev_guarded(bh_params *params, const bh_r1cs *r1cs, const void *inputs_dev, size_t in_stride,
                                    const void *aux_dev, size_t aux_stride, size_t k, const void *r, const void *s, unsigned flags,
                                    void *stream, void *proofs_out, int32_t *rcs, uint32_t *first_unsatisfied, float *timings4,
                                    size_t workspace_budget, int mode) {
  using namespace groth16;
  if (!params || !r1cs) return BH_ERR_INVALID_ARG;
  if (k && (!r || !s || !proofs_out || !rcs)) return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  const int rc = guarded([&] {
    R1csView view(r1cs);
    std::vector<Fr> rr(k), ss(k);
    if (k) { memcpy(rr.data(), r, k * 32); memcpy(ss.data(), s, k * 32); }
    std::vector<Proof> proofs(k);
    std::vector<int> codes(k, BH_OK);
    prove_witness_batch_dev_codes(view.r, *params->p, DeviceWitnesses{inputs_dev, in_stride, aux_dev, aux_stride, k}, rr.data(),
                                  ss.data(), flags, stream, proofs.data(), codes.data(), first_unsatisfied, &tm, workspace_budget, mode);
    write_results(proofs, codes, proofs_out, rcs);
    return BH_OK;
  });
  write_timings(timings4, tm);
  return rc;
}

// bh_groth16_prove_witness_batch (and _checked), and the test library's twins with a workspace budget and a mode of their own
int prove_witness_batch_guarded(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs, const void *aux,
                                size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out, int32_t *rcs,
                                float *timings4, size_t workspace_budget, int mode, bool checked, uint32_t *first_unsatisfied) {
  using namespace groth16;
  if (!params || !r1cs) return BH_ERR_INVALID_ARG;
  if (k && (!r || !s || !proofs_out || !rcs || (n_inputs && !inputs) || (n_aux && !aux))) return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  const int rc = guarded([&] {
    R1csView view(r1cs);
    // caller records may be unaligned: copied then (the witnesses of a large circuit are tens of megabytes each - an
    // aligned caller's arrays are read in place)
    std::vector<Fr> in, ax, rr(k), ss(k);
    const Fr *in_p = (const Fr *)inputs, *ax_p = (const Fr *)aux;
    if ((uintptr_t)inputs % alignof(Fr) && k * n_inputs) { in.resize(k * n_inputs); memcpy(in.data(), inputs, k * n_inputs * 32); in_p = in.data(); }
    if ((uintptr_t)aux % alignof(Fr) && k * n_aux) { ax.resize(k * n_aux); memcpy(ax.data(), aux, k * n_aux * 32); ax_p = ax.data(); }
    if (k) { memcpy(rr.data(), r, k * 32); memcpy(ss.data(), s, k * 32); }
    std::vector<WitnessView> ws(k);
    for (size_t j = 0; j < k; j++) ws[j] = WitnessView{in_p + j * n_inputs, n_inputs, ax_p + j * n_aux, n_aux};
    std::vector<Proof> proofs(k);
    std::vector<int> codes(k, BH_OK);
    if (checked)   // bh_groth16_prove_witness_batch_checked: the check pre-pass, then the satisfied witnesses as below
      prove_witness_batch_checked_codes(view.r, *params->p, ws.data(), k, rr.data(), ss.data(), proofs.data(), codes.data(),
                                        first_unsatisfied, &tm, workspace_budget, mode);
    else
      prove_witness_batch_codes(view.r, *params->p, ws.data(), k, rr.data(), ss.data(), proofs.data(), codes.data(), &tm, workspace_budget, mode);
    write_results(proofs, codes, proofs_out, rcs);
    return BH_OK;
  });
  write_timings(timings4, tm);
  return rc;
}
