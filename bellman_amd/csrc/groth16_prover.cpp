// groth16::create_proof and friends: linear-combination evaluation during synthesis, the eight
// multiexps + h block on the device, proof assembly, the R1CS capture, the witness-only path and the
// async pipeline.  k proofs in one call: groth16_batch.cpp.  Reference map in groth16.hpp.
#include <string.h>

#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "groth16_internal.hpp"

namespace groth16 {
using namespace bellman;
using namespace detail;

// ---- prover.rs:19-55 ------------------------------------------------------------------------------
static inline Fr eval(const LinearCombination &lc, DensityTracker *input_density, DensityTracker *aux_density,
                      const std::vector<Fr> &input_assignment, const std::vector<Fr> &aux_assignment) {
  Fr acc = Fr::zero();
  const Fr one = Fr::one();
  const size_t n = lc.size();
  for (size_t t = 0; t < n; t++) {
    const Variable &var = lc[t].first;
    const Fr &coeff = lc[t].second;
    if (coeff.is_zero()) continue;          // zero coefficients count for neither value nor density (:31)
    const Fr *value;
    if (var.kind() == Index::Input) {
      value = &input_assignment[var.idx()];
      if (input_density) input_density->inc(var.idx());
    } else {
      value = &aux_assignment[var.idx()];
      if (aux_density) aux_density->inc(var.idx());
    }
    // most terms carry the coefficient one (`lc + x`), then the ubiquitous `(c, CS::one())` terms: value one
    if (coeff == one) acc = acc + *value;
    else if (*value == one) acc = acc + coeff;
    else acc = acc + *value * coeff;
  }
  return acc;
}

// ---- recycled assignments ----------------------------------------------------------------------------------------
// A 2^20-constraint ProvingAssignment is five vectors of 32 MiB.  Grown by push_back from empty and freed after every
// proof they cost reallocation copies and ~40 000 first-touch page faults per proof - a third of the synthesis time
// (profiles/archive/r3_host_synthesis.txt).  Finished assignments are cleared (capacity kept) and handed to the next proof.
namespace {
template <class T>
class Recycler {
 public:
  std::unique_ptr<T> get() {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (!free_.empty()) {
        std::unique_ptr<T> p = std::move(free_.back());
        free_.pop_back();
        return p;
      }
    }
    return std::unique_ptr<T>(new T());
  }
  void put(std::unique_ptr<T> p) {
    if (!p) return;
    reset(*p);
    std::lock_guard<std::mutex> g(mu_);
    if (free_.size() < 16) free_.push_back(std::move(p));   // at most 16 idle assignments are kept
  }

 private:
  static void reset(ProvingAssignment &a) {
    a.a.clear(); a.b.clear(); a.c.clear(); a.input_assignment.clear(); a.aux_assignment.clear();
    a.a_aux_density.clear(); a.b_input_density.clear(); a.b_aux_density.clear();
  }
  static void reset(WitnessAssignment &w) { w.input_assignment.clear(); w.aux_assignment.clear(); }
  std::mutex mu_;
  std::vector<std::unique_ptr<T>> free_;
};
Recycler<ProvingAssignment> g_assignments;
Recycler<WitnessAssignment> g_witnesses;
template <class T>
struct Recycled {   // returns the object to its pool on scope exit, exceptions included
  Recycler<T> &pool;
  std::unique_ptr<T> p;
  explicit Recycled(Recycler<T> &r) : pool(r), p(r.get()) {}
  ~Recycled() { pool.put(std::move(p)); }
  T &operator*() { return *p; }
};
}  // namespace
AsyncProof::~AsyncProof() {
  if (worker.joinable()) worker.join();
  g_assignments.put(std::move(assignment));
  g_witnesses.put(std::move(witness));
}

// ---- prover.rs:73-162 -----------------------------------------------------------------------------
Variable ProvingAssignment::alloc(ValueFn f) {
  aux_assignment.push_back(f());
  a_aux_density.add_element();
  b_aux_density.add_element();
  return Variable::new_unchecked(Index::Aux, aux_assignment.size() - 1);
}
Variable ProvingAssignment::alloc_input(ValueFn f) {
  input_assignment.push_back(f());
  b_input_density.add_element();
  return Variable::new_unchecked(Index::Input, input_assignment.size() - 1);
}
void ProvingAssignment::enforce(const LcFn &fa, const LcFn &fb, const LcFn &fc) {
  // inputs have full density in the A query; there is no C query (prover.rs:119-141).  The closures get combinations
  // that evaluate each term as it is added (groth16.hpp); a closure that returns some other, stored combination is
  // evaluated the classic way.  CONTRACT of the evaluating form (the reference's `eval` walks only the RETURNED
  // combination, prover.rs:19-55): a closure returns a combination derived linearly from its argument - terms added to a
  // copy that is then discarded would still count in the value and in the density maps (the accumulator lives in the sink,
  // groth16.hpp LcSink::acc) - or a stored combination built without touching the argument.  Every closure of the
  // reference's own circuits and gadgets has the first shape (`|lc| lc + a + (c, b)`).
  const std::vector<Fr> *in = &input_assignment, *ax = &aux_assignment;
  const LcSink sa{in, ax, nullptr, &a_aux_density}, sb{in, ax, &b_input_density, &b_aux_density}, sc{in, ax, nullptr, nullptr};
  // (the value goes from the combination's accumulator into the vector's new slot limb by limb: handed on as an Fr it is
  //  copied with 16-byte loads from the 8-byte stores of the last addition, which the store buffer cannot forward -
  //  a tenth of the synthesis time of a 2^20-constraint circuit, tools/host_profile.py)
  auto run = [&](const LcFn &f, const LcSink &sink, std::vector<Fr> &out) {
    const LinearCombination r = f(LinearCombination::evaluating(&sink));
    // a closure compiled with BELLMAN_HIP_CHECK_CLOSURES counted every term it added to any copy of its argument: the
    // returned combination must carry exactly those (prover.rs:19-55 evaluates the returned combination and nothing else)
    if (sink.pushed && (!r.is_evaluating() || r.size() != sink.pushed))
      throw std::invalid_argument("enforce: the closure added terms to a copy of its argument that it did not return");
    out.emplace_back();
    if (r.is_evaluating()) r.value_into(out.back());
    else out.back() = eval(r, sink.input_density, sink.aux_density, input_assignment, aux_assignment);
  };
  run(fa, sa, a);
  run(fb, sb, b);
  run(fc, sc, c);
}

// (the h block is a short dependent chain on the proof's critical path - the H multiexp waits for it.  A high-priority
// stream for it was measured: no gain for one proof and 8 % less throughput with twelve proofs in flight,
// profiles/archive/r3_call3_oversub.txt)
detail::ProofStream::ProofStream(bh_ctx *c) : ctx(c) { check(bh_stream_create_priority(ctx, 0, &st)); }
detail::ProofStream::~ProofStream() { if (st) { (void)bh_stream_synchronize(ctx, st); (void)bh_stream_destroy(ctx, st); } }
namespace {
template <class A> A add_pts(int group, const A &x, const A &y) { A r; bh_point_add(group, &r, &x, &y, 1); return r; }
template <class A> A mul_pt(int group, const A &x, const Fr &k) {
  uint64_t kc[4];
  k.to_canonical(kc);
  A r;
  bh_point_mul(group, &r, &x, kc);
  return r;
}
}  // namespace

// ---- prover.rs:217-360 ----------------------------------------------------------------------------
namespace {
// The slice of an n-term multiexp that part `k` of `parts` computes when one proof is spread over
// several GPUs: contiguous in the scalar index, cut at multiples of 64 so that the
// density bitmap of the slice starts on a word.  parts = 1 gives [0, n).
struct Slice { size_t lo, hi; };
Slice slice_of(size_t n, size_t part, size_t parts) {
  auto cut = [&](size_t k) {
    if (k >= parts) return n;
    const size_t c = (size_t)((unsigned __int128)n * k / parts) & ~size_t(63);
    return c < n ? c : n;
  };
  return Slice{cut(part), cut(part + 1)};
}
}  // namespace

// test hook (host only): the slice of an n-term multiexp part `part` of `parts` computes
void proof_slice_for_tests(size_t n, size_t part, size_t parts, size_t *lo, size_t *hi) {
  const Slice sl = slice_of(n, part, parts);
  *lo = sl.lo;
  *hi = sl.hi;
}

// prover.rs:217-318 + the waits of :339-354: the eight multiexp results (of this part's slices)
void detail::msm_sums(const AssignmentSource &src, Parameters &params, size_t part, size_t parts, MsmSums &out, ProveTimings *tm) {
  bh_ctx *ctx = params.ctx;
  const double t0 = now_ms();
  const size_t n_cons = src.n_cons;
  const Domain dom = domain_of(n_cons);
  const size_t m = dom.m;
  const uint32_t log_m = dom.log_m;
  // assignments: uploaded once, shared by seven multiexps (prover.rs:248-318)
  const size_t n_in = src.n_in, n_aux = src.n_aux;
  std::unique_ptr<DevBuf> own_in, own_aux;   // (none for a witness that is resident already)
  if (!src.resident) {
    own_in.reset(new DevBuf(ctx, n_in * 32 + 32));
    own_aux.reset(new DevBuf(ctx, n_aux * 32 + 32));
  }
  const void *const d_in = src.resident ? src.inputs_dev : own_in->p, *const d_aux = src.resident ? src.aux_dev : own_aux->p;
  ProofStream ps(ctx);
  if (!src.resident) {
    check(bh_dev_upload_on(ctx, own_in->p, src.inputs, n_in * 32, ps.st));
    if (n_aux) check(bh_dev_upload_on(ctx, own_aux->p, src.aux, n_aux * 32, ps.st));
  }
  Densities dens;
  if (src.host) {
    dens.on_host(src.a_aux_density, src.b_input_density, src.b_aux_density, n_in);
    dens.upload(ctx, n_in, n_aux, ps.st);
  } else {
    dens.of(*src.r1cs);
  }
  const QueryTable queries_of = queries(params, n_in, dens.b_in_total);

  BH_TRACE("prove_core start: uploads queued");
  check(bh_stream_synchronize(ctx, ps.st));   // the multiexp jobs run on their own streams
  BH_TRACE("assignment resident");
  // h-block buffers are declared here so that `jobs` (declared after every buffer a job reads) is
  // destroyed first and drains whatever is still in flight if an exception unwinds this frame
  DevBuf da(ctx, m * 32), db(ctx, m * 32), dc(ctx, m * 32);
  StreamDrain drain{ps};
  InFlight<bh_msm_job> jobs(N_SLOTS);
  DevBuf dscratch(ctx, log_m > 11 ? m * 32 : 32);   // FFT ping-pong vector of the h block
  StreamDrain drain2{ps};                            // (drains before dscratch is released)
  // (A two-phase issue - BH_MSM_HOLD / bh_msm_start: first every job's digit + sort stage, then the bucket accumulations in
  // chain order - was measured for proofs above 2^16 and is not used: no gain for one proof and 12 % less throughput with
  // twelve in flight, the sorts of one proof no longer fill the gaps of another; profiles/archive/r3_call6_hold_ab.txt.)
  // one multiexp over this part's slice of the slot's scalars: the bases advance by what the skipped scalars would have
  // consumed (all of them without a density map, the set bits with one)
  struct SlotSlice { const Query &q; const void *scalars_dev; Slice sl; size_t base_skip; };
  auto slice_for = [&](Slot slot) {
    const Query &q = queries_of[slot];
    const size_t n = q.scalars == FROM_INPUTS ? n_in : q.scalars == FROM_AUX ? n_aux : m - 1;   // a.len() - 1, :238-244
    const void *dev = q.scalars == FROM_INPUTS ? d_in : q.scalars == FROM_AUX ? d_aux : da.p;
    const Slice sl = slice_of(n, part, parts);
    return SlotSlice{q, dev, sl, q.skip + (q.density >= 0 ? popcount_bits(dens.host_of(q.density), sl.lo) : sl.lo)};
  };
  auto issue = [&](Slot slot) {
    const SlotSlice s = slice_for(slot);
    const size_t n = s.sl.hi - s.sl.lo;
    const uint64_t *dens_dev = dens.dev_of(s.q.density), *dens_host = dens.host_of(s.q.density);
    if (s.q.scalars == FROM_INPUTS && n <= HOST_INPUTS_MAX && src.inputs) {   // (one or two terms: answered on the host)
      check(bh_msm_async(ctx, s.q.bases, s.base_skip, (const char *)src.inputs + s.sl.lo * 32, n, BH_SCALARS_MONT,
                         dens_host ? dens_host + s.sl.lo / 64 : nullptr, dens_host ? n : 0, &jobs.at[slot]));
      BH_TRACE("  multiexp of %zu terms answered on the host", n);
      return;
    }
    check(bh_msm_async_dev(ctx, s.q.bases, s.base_skip, (const char *)s.scalars_dev + s.sl.lo * 32, n, BH_SCALARS_MONT,
                           dens_dev ? dens_dev + s.sl.lo / 64 : nullptr, dens_dev ? n : 0, &jobs.at[slot]));
    BH_TRACE("  multiexp of %zu terms issued", n);
  };
  auto issue_seven = [&] { for (Slot slot : ISSUE_ORDER) issue(slot); };
  // h block (prover.rs:221-245), enqueue only: a, b, c stay in HBM; the quotient's coefficients are consumed by the
  // H multiexp straight from device memory (no host round trip, no serial Fr -> Exponent pass)
  auto enqueue_h_block = [&] {
    if (src.host) {
      // EvaluationDomain::from_coeffs pads with zeros (domain.rs:68): the padding is written on the device
      const Fr *ev[3] = {src.a, src.b, src.c};
      void *dst[3] = {da.p, db.p, dc.p};
      for (int i = 0; i < 3; i++) {
        if (m > n_cons) check(bh_dev_zero_on(ctx, (char *)dst[i] + n_cons * 32, (m - n_cons) * 32, ps.st));
        check(bh_dev_upload_on(ctx, dst[i], ev[i], n_cons * 32, ps.st));
      }
    } else {
      // a = A.w, b = B.w, c = C.w straight into the FFT buffers (prover.rs:19-55,105-145 on the device)
      check(bh_r1cs_eval_dev(ctx, src.r1cs->handle, d_in, d_aux, da.p, db.p, dc.p, log_m, ps.st));
    }
    check(bh_h_poly_fr_dev_on(ctx, da.p, db.p, dc.p, dscratch.p, log_m, ps.st));
  };
  // The seven multiexps that only need the assignments and the h block are independent: the order of issue is
  // unobservable (the order of waits is kept, prover.rs:339-354).  Large proofs issue the multiexps first, so the
  // GPU is busy while the host stages a/b/c; small proofs (a few launches of latency-bound kernels each) put the h
  // block's dozen kernels at the head of the hardware queues instead of behind ~100 multiexp launches.
  // A small proof is bound by the HOST: every job is ~20 kernel launches, ~0.2 ms of API time, and the H multiexp can
  // only be issued once the h block has run (profiles/archive/r2_call21_mimc_timeline.txt: five jobs issued one after the other,
  // the last at 0.97 ms of a 1.62 ms GPU span).  So the seven assignment multiexps are enqueued by a helper thread while
  // this one enqueues the h block, waits for it and issues H.
  double t1;
  if (log_m <= 16) {
    std::exception_ptr helper_error;
    std::thread helper([&] {
      try { issue_seven(); } catch (...) { helper_error = std::current_exception(); }
    });
    try {
      enqueue_h_block();
      BH_TRACE("h block enqueued");
      check(bh_stream_synchronize(ctx, ps.st));
      t1 = now_ms();
      issue(H);
    } catch (...) {
      helper.join();
      throw;
    }
    helper.join();
    if (helper_error) std::rethrow_exception(helper_error);
  } else {
    // The H multiexp is ordered after the h block by an event (bh_msm_async_dev_after): the host never waits between
    // them.  With the constraints evaluated on the device the h block is enqueued FIRST - nothing on the host delays it,
    // and started late it queues behind the multiexps' long kernels, the H multiexp then runs alone at the end
    // (profiles/archive/r3_call2_proof_timeline.txt).  With host evaluations the multiexps go first: the GPU works while the
    // host stages a, b, c (96 MiB of pageable memory at 2^20).  H comes last, by which time the h block has long finished
    // beside the others.
    if (!src.host) {
      enqueue_h_block();
      // the accumulations wait for the h block (their digit / sort stages run beside it): behind the G2 accumulation's
      // 5 ms workgroups an FFT pass waits for a free SIMD, and the h block took 17 ms (profiles/archive/r3_call4_proof_timeline.txt)
      check(bh_ctx_accumulations_after(ctx, ps.st));
    }
    issue_seven();
    if (src.host) enqueue_h_block();
    const SlotSlice h = slice_for(H);
    check(bh_msm_async_dev_after(ctx, h.q.bases, h.base_skip, (const char *)h.scalars_dev + h.sl.lo * 32, h.sl.hi - h.sl.lo,
                                 BH_SCALARS_MONT, nullptr, 0, nullptr, ps.st, &jobs.at[H]));
    BH_TRACE("7 multiexps + h block + H issued; n_cons=%zu m=%zu", n_cons, m);
    t1 = now_ms();
  }

  BH_TRACE("all msm issued n_in=%zu n_aux=%zu", n_in, n_aux);
  wait_eight(jobs, params, out);
  if (tm) {
    tm->h_poly_ms = (float)(t1 - t0);
    tm->msm_ms = (float)(now_ms() - t1);
    tm->total_ms = (float)(now_ms() - t0);
  }
}

// prover.rs:320-338: the part of the proof elements that depends on the verifying key and r, s only
static ProofBlinding blind_terms(const Parameters &params, const Fr &r, const Fr &s) {
  const VerifyingKey &vk = params.vk;
  if (subverted(params)) throw SynthesisError(BH_ERR_UNEXPECTED_IDENTITY, "UnexpectedIdentity");
  ProofBlinding b;
  b.g_a = add_pts(BH_G1, mul_pt(BH_G1, vk.delta_g1, r), vk.alpha_g1);   // :326-327
  b.g_b = add_pts(BH_G2, mul_pt(BH_G2, vk.delta_g2, s), vk.beta_g2);    // :328-329
  const Fr rs = r * s;
  b.g_c = mul_pt(BH_G1, vk.delta_g1, rs);                                // :331-338
  b.g_c = add_pts(BH_G1, b.g_c, mul_pt(BH_G1, vk.alpha_g1, s));
  b.g_c = add_pts(BH_G1, b.g_c, mul_pt(BH_G1, vk.beta_g1, r));
  return b;
}
// prover.rs:339-360: fold the multiexp results in
Proof detail::finish_proof(const ProofBlinding &b, const MsmSums &m, const Fr &r, const Fr &s) {
  // g_a = blind + a_answer; g_b = blind + b_g2_answer; g_c = blind + [s] a_answer + [r] b_g1_answer + h + l with
  // a_answer = a_inputs + a_aux etc. - each as ONE host linear combination (shared doubling chain, one inversion)
  const uint64_t one[4] = {1, 0, 0, 0};
  uint64_t rc[4], sc[4];
  r.to_canonical(rc);
  s.to_canonical(sc);
  Proof p;
  {
    const G1Affine pts[3] = {b.g_a, m.a_in, m.a_aux};                                              // :339-343
    bh_point_lincomb(BH_G1, &p.a, pts, nullptr, 3);
  }
  {
    const G2Affine pts[3] = {b.g_b, m.b2_in, m.b2_aux};                                            // :347-350
    bh_point_lincomb(BH_G2, &p.b, pts, nullptr, 3);
  }
  {
    const G1Affine pts[7] = {b.g_c, m.a_in, m.a_aux, m.b1_in, m.b1_aux, m.h, m.l};                 // :342, 351-354
    uint64_t ks[7][4];
    const uint64_t *src[7] = {one, sc, sc, rc, rc, one, one};
    for (int i = 0; i < 7; i++) memcpy(ks[i], src[i], 32);
    bh_point_lincomb(BH_G1, &p.c, pts, ks, 7);
  }
  return p;
}
Proof assemble_proof(const Parameters &params, const MsmSums &m, const Fr &r, const Fr &s) {
  return finish_proof(blind_terms(params, r, s), m, r, s);
}

// prover.rs:320-360 for k proofs on the device (bh_proof_finish_dev): sums, r, s and proofs are device buffers, the call
// returns when the proofs are written.  An identity delta is the caller's to refuse.
int finish_proofs_dev(const Parameters &params, const void *sums_dev, const void *r_dev, const void *s_dev, size_t k,
                      void *proofs_dev, void *stream) {
  const VerifyingKey &vk = params.vk;
  unsigned char vk5[BH_FINISH_KEY_BYTES];
  memcpy(vk5, &vk.alpha_g1, 96); memcpy(vk5 + 96, &vk.beta_g1, 96); memcpy(vk5 + 192, &vk.beta_g2, 192);
  memcpy(vk5 + 384, &vk.delta_g1, 96); memcpy(vk5 + 480, &vk.delta_g2, 192);
  return bh_proof_finish_dev(params.ctx, vk5, sums_dev, r_dev, s_dev, k, proofs_dev, stream);
}
std::vector<Proof> assemble_proofs(const Parameters &params, const MsmSums *sums, const Fr *r, const Fr *s, size_t k) {
  std::vector<Proof> proofs(k);
  if (!k) return proofs;
  if (subverted(params)) throw SynthesisError(BH_ERR_UNEXPECTED_IDENTITY, "UnexpectedIdentity");
  bh_ctx *ctx = params.ctx;
  static_assert(sizeof(MsmSums) == BH_MSM_SUMS_BYTES && sizeof(Proof) == 384 && sizeof(Fr) == 32, "record sizes");
  DevBuf d_sums(ctx, k * sizeof(MsmSums)), d_rs(ctx, k * 64), d_proofs(ctx, k * sizeof(Proof));
  void *d_s = (char *)d_rs.p + k * 32;
  try {
    check(bh_dev_upload(ctx, d_sums.p, sums, k * sizeof(MsmSums)));
    check(bh_dev_upload(ctx, d_rs.p, r, k * 32));
    check(bh_dev_upload(ctx, d_s, s, k * 32));
    check(finish_proofs_dev(params, d_sums.p, d_rs.p, d_s, k, d_proofs.p, nullptr));
    check(bh_dev_download(ctx, proofs.data(), d_proofs.p, k * sizeof(Proof)));
  } catch (...) {
    // what is queued on the context's stream finishes before the three buffers return to the pool as this frame unwinds
    (void)bh_stream_synchronize(ctx, nullptr);
    throw;
  }
  return proofs;
}

void MsmSums::add(const MsmSums &o) {
  a_in = add_pts(BH_G1, a_in, o.a_in); a_aux = add_pts(BH_G1, a_aux, o.a_aux);
  b1_in = add_pts(BH_G1, b1_in, o.b1_in); b1_aux = add_pts(BH_G1, b1_aux, o.b1_aux);
  b2_in = add_pts(BH_G2, b2_in, o.b2_in); b2_aux = add_pts(BH_G2, b2_aux, o.b2_aux);
  h = add_pts(BH_G1, h, o.h); l = add_pts(BH_G1, l, o.l);
}

detail::Blinding::Blinding(const Parameters &params, const Fr *r, const Fr *s, size_t k) : terms(k) {
  const size_t n_threads = std::min<size_t>(k, 8);
  for (size_t t = 0; t < n_threads; t++)
    threads_.emplace_back([this, &params, r, s, k, t, n_threads] {
      try {
        for (size_t j = t; j < k; j += n_threads) terms[j] = blind_terms(params, r[j], s[j]);
      } catch (...) {
        std::lock_guard<std::mutex> g(mu_);
        if (!error) error = std::current_exception();
      }
    });
}

static Proof prove_core(const AssignmentSource &src, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  const double t0 = now_ms();
  MsmSums sums;
  Blinding blind(params, &r, &s, 1);
  std::exception_ptr msm_err;
  try {
    msm_sums(src, params, 0, 1, sums, tm);
  } catch (...) {
    msm_err = std::current_exception();   // every job has been drained by now (InFlight)
  }
  blind.join();
  // an identity delta takes precedence over whatever a multiexp reports (first_failure, groth16_internal.hpp)
  if (blind.error) std::rethrow_exception(blind.error);
  if (msm_err) std::rethrow_exception(msm_err);
  Proof p = finish_proof(blind.terms[0], sums, r, s);
  if (tm) tm->total_ms = (float)(now_ms() - t0);
  return p;
}

void detail::require_shape(const R1cs &r1cs, const WitnessView *witnesses, size_t k) {
  for (size_t j = 0; j < k; j++)
    if (witnesses[j].n_inputs != r1cs.num_inputs || witnesses[j].n_aux != r1cs.num_aux)
      throw std::invalid_argument("witness does not have the shape of the captured circuit");
}
static AssignmentSource resident_source(const R1cs &r1cs, const Fr *inputs, size_t n_inputs, const Fr *aux, size_t n_aux) {
  const WitnessView w{inputs, n_inputs, aux, n_aux};
  require_shape(r1cs, &w, 1);
  AssignmentSource src;
  src.inputs = inputs; src.n_in = n_inputs;
  src.aux = aux; src.n_aux = n_aux;
  src.n_cons = r1cs.num_constraints;
  src.r1cs = &r1cs;
  return src;
}

MsmSums prove_witness_part(const R1cs &r1cs, Parameters &params, const Fr *inputs, size_t n_inputs, const Fr *aux, size_t n_aux,
                           size_t part, size_t parts, ProveTimings *tm) {
  if (parts == 0 || part >= parts) throw std::invalid_argument("bad part");
  MsmSums sums;
  msm_sums(resident_source(r1cs, inputs, n_inputs, aux, n_aux), params, part, parts, sums, tm);
  return sums;
}

Proof prove_assignment(ProvingAssignment &prover, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  AssignmentView v;
  v.a = prover.a.data(); v.b = prover.b.data(); v.c = prover.c.data(); v.n_constraints = prover.a.size();
  v.input_assignment = prover.input_assignment.data(); v.n_inputs = prover.input_assignment.size();
  v.aux_assignment = prover.aux_assignment.data(); v.n_aux = prover.aux_assignment.size();
  v.a_aux_density = prover.a_aux_density.words(); v.b_input_density = prover.b_input_density.words();
  v.b_aux_density = prover.b_aux_density.words();
  return prove_assignment(v, params, r, s, tm);
}
Proof prove_assignment(const AssignmentView &v, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  AssignmentSource src;
  src.inputs = v.input_assignment; src.n_in = v.n_inputs;
  src.aux = v.aux_assignment; src.n_aux = v.n_aux;
  src.n_cons = v.n_constraints;
  src.host = true;
  src.a = v.a; src.b = v.b; src.c = v.c;
  src.a_aux_density = v.a_aux_density; src.b_input_density = v.b_input_density; src.b_aux_density = v.b_aux_density;
  return prove_core(src, params, r, s, tm);
}

Proof prove_witness(const R1cs &r1cs, Parameters &params, const Fr *inputs, size_t n_inputs, const Fr *aux, size_t n_aux,
                    const Fr &r, const Fr &s, ProveTimings *tm) {
  return prove_core(resident_source(r1cs, inputs, n_inputs, aux, n_aux), params, r, s, tm);
}

// ---- the witnesses of k proofs into device memory, and their check (the k-proof paths: groth16_batch.cpp) ----------
void detail::upload_witnesses(bh_ctx *ctx, const WitnessView *w, size_t g, void *d_in, void *d_aux, void *st, bool coalesce) {
  const size_t n_in = w[0].n_inputs, n_aux = w[0].n_aux, in_stride = n_in * 32, aux_stride = n_aux * 32;
  bool adjacent = coalesce;
  for (size_t j = 0; adjacent && j + 1 < g; j++)
    adjacent = w[j + 1].inputs == w[j].inputs + n_in && w[j + 1].aux == w[j].aux + n_aux;
  if (adjacent) {
    if (n_in) check(bh_dev_upload_on(ctx, d_in, w[0].inputs, g * in_stride, st));
    if (n_aux) check(bh_dev_upload_on(ctx, d_aux, w[0].aux, g * aux_stride, st));
    return;
  }
  for (size_t j = 0; j < g; j++) {
    if (n_in) check(bh_dev_upload_on(ctx, (char *)d_in + j * in_stride, w[j].inputs, in_stride, st));
    if (n_aux) check(bh_dev_upload_on(ctx, (char *)d_aux + j * aux_stride, w[j].aux, aux_stride, st));
  }
}

std::vector<uint32_t> detail::check_witnesses(bh_ctx *ctx, const R1cs &r1cs, const WitnessView *witnesses, size_t k, size_t budget) {
  require_shape(r1cs, witnesses, k);
  if (!ctx) throw std::invalid_argument("the R1cs handle was adopted without its context");
  std::vector<uint32_t> first_bad(k, BH_R1CS_SATISFIED);
  if (!k) return first_bad;
  const size_t in_stride = r1cs.num_inputs * 32, aux_stride = r1cs.num_aux * 32;
  const size_t group = std::min(k, std::max<size_t>(budget / (in_stride + aux_stride + 4), 1));
  for (size_t first = 0; first < k; first += group) {
    const size_t g = std::min(group, k - first);
    DevBuf d_in(ctx, g * in_stride + 32), d_aux(ctx, g * aux_stride + 32), d_bad(ctx, g * sizeof(uint32_t));
    ProofStream ps(ctx);
    StreamDrain drain{ps};
    upload_witnesses(ctx, witnesses + first, g, d_in.p, d_aux.p, ps.st, true);
    check(bh_r1cs_check_many_dev(ctx, r1cs.handle, d_in.p, in_stride, d_aux.p, aux_stride, g, (uint32_t *)d_bad.p, ps.st));
    check(bh_stream_synchronize(ctx, ps.st));
    check(bh_dev_download(ctx, first_bad.data() + first, d_bad.p, g * sizeof(uint32_t)));
  }
  return first_bad;
}

// ---- structure capture (generator.rs:43-131 KeypairAssembly, plus the input rows of prover.rs:208-215)
namespace {
struct FrHash {
  size_t operator()(const Fr &f) const {
    uint64_t h = f.l[0] * 0x9E3779B97F4A7C15ULL;
    h ^= f.l[1] + 0xBF58476D1CE4E5B9ULL + (h << 6) + (h >> 2);
    h ^= f.l[2] + 0x94D049BB133111EBULL + (h << 6) + (h >> 2);
    h ^= f.l[3] + (h << 6) + (h >> 2);
    return (size_t)h;
  }
};
class ShapeAssembly : public ConstraintSystem {
 public:
  size_t num_inputs = 0, num_aux = 0;
  // the matrices in the layout bh_r1cs_create takes (CSR: row_ptr, variable, coefficient-table index), written once.  A
  // variable is stored as its index with AUX_BIT for an aux variable until the capture ends: only then is the number
  // of inputs known, and `finish` turns every entry into its column (inputs first, then aux) in place.
  static constexpr uint32_t AUX_BIT = 0x80000000u;
  std::vector<uint32_t> row_ptr[3], var[3], coeff[3];
  static uint32_t pack(const Variable &v) { return (uint32_t)v.idx() | (v.kind() == Index::Aux ? AUX_BIT : 0u); }
  void finish() {
    const uint32_t ni = (uint32_t)num_inputs;
    for (auto &vm : var)
      for (uint32_t &x : vm) x = (x & AUX_BIT) ? ni + (x & ~AUX_BIT) : x;
  }
  std::vector<Fr> coeffs;
  // Coefficients are shared through a direct-mapped cache of table indices, not an exact map: a circuit's constants
  // (round constants, powers of two) repeat and hit; a circuit whose coefficients are all different (the synthetic
  // chain: 2 new ones per constraint) pays one compare and one append per term instead of a node allocation and a
  // rehash - the one-time capture of 2^20 constraints 1.32 -> 0.42 s in the build container (bh_test_capture_check).  A collision only stores a
  // constant twice (the table may hold duplicates: terms carry an index, csrc/r1cs.hip).
  // A cache entry is (32 hash bits | table index): the stored coefficient is only looked at when the hash bits agree - for a
  // circuit of distinct coefficients every probe would otherwise be a cache miss into a table of tens of megabytes.
  static constexpr size_t CACHE_SLOTS = size_t(1) << 16;
  std::vector<uint64_t> coeff_cache;
  const Fr one_ = Fr::one();
  ShapeAssembly() : coeff_cache(CACHE_SLOTS, 0) {   // 0 = the constant one (never looked up): an empty slot
    coeffs.push_back(Fr::one());
    for (auto &rp : row_ptr) rp.push_back(0);
  }
  Variable alloc(ValueFn) override { return Variable::new_unchecked(Index::Aux, num_aux++); }
  Variable alloc_input(ValueFn) override { return Variable::new_unchecked(Index::Input, num_inputs++); }
  void add_term(int m, const Variable &v, const Fr &k) {
    if (k.is_zero()) return;     // prover.rs:31: no value, no density
    if (k == one_) {             // the usual `lc + x` term: coefficient table entry 0, no hash lookup
      var[m].push_back(pack(v)); coeff[m].push_back(0);
      return;
    }
    const uint64_t h = FrHash()(k);
    uint64_t &entry = coeff_cache[h & (CACHE_SLOTS - 1)];
    const uint64_t tag = h & 0xffffffff00000000ULL;
    uint32_t slot = (uint32_t)entry;
    if (slot == 0 || (entry & 0xffffffff00000000ULL) != tag || !(coeffs[slot] == k)) {
      slot = (uint32_t)coeffs.size();
      entry = tag | slot;
      coeffs.push_back(k);
    }
    var[m].push_back(pack(v)); coeff[m].push_back(slot);
  }
  struct Hooked { ShapeAssembly *cs; int m; };
  static void hook(void *self, Variable v, const Fr &k) {
    Hooked *h = static_cast<Hooked *>(self);
    h->cs->add_term(h->m, v, k);
  }
  void enforce(const LcFn &fa, const LcFn &fb, const LcFn &fc) override {
    // the closures get combinations whose terms go straight into the matrices (LcSink::hook); a closure that returns
    // some other, stored combination is walked the classic way
    const LcFn *fs[3] = {&fa, &fb, &fc};
    for (int m = 0; m < 3; m++) {
      Hooked h{this, m};
      LcSink sink{nullptr, nullptr, nullptr, nullptr, &ShapeAssembly::hook, &h};
      const LinearCombination r = (*fs[m])(LinearCombination::evaluating(&sink));
      if (sink.pushed && (!r.is_evaluating() || r.size() != sink.pushed))   // (checking builds: see ProvingAssignment::enforce)
        throw std::invalid_argument("enforce: the closure added terms to a copy of its argument that it did not return");
      if (!r.is_evaluating())
        for (size_t i = 0; i < r.size(); i++) add_term(m, r[i].first, r[i].second);
      row_ptr[m].push_back((uint32_t)var[m].size());
    }
  }
};
}  // namespace

// the input rows of prover.rs:208-215: one constraint `input_i * 0 = 0` per input
static void enforce_input_rows(ConstraintSystem &cs, size_t num_inputs) {
  for (size_t i = 0; i < num_inputs; i++) {
    cs.enforce([i](LinearCombination lc) { return lc + Variable::new_unchecked(Index::Input, i); },
               [](LinearCombination lc) { return lc; }, [](LinearCombination lc) { return lc; });
  }
}
// prover.rs:182-215: `circuit` into a ProvingAssignment (the constant one first), the input rows appended
static void synthesize_assignment(Circuit &circuit, ProvingAssignment &pa) {
  pa.alloc_input([] { return Fr::one(); });
  circuit.synthesize(pa);
  enforce_input_rows(pa, pa.input_assignment.size());
}
void synthesize_witness(Circuit &circuit, const R1cs &r1cs, WitnessAssignment &w) {
  w.input_assignment.reserve(r1cs.num_inputs);
  w.aux_assignment.reserve(r1cs.num_aux);
  w.alloc_input([] { return Fr::one(); });
  circuit.synthesize(w);
}

// the circuit's shape with the input rows of prover.rs:208-215 appended
static void capture_shape(Circuit &shape_of, ShapeAssembly &cs) {
  cs.alloc_input([] { return Fr::one(); });
  shape_of.synthesize(cs);
  enforce_input_rows(cs, cs.num_inputs);
  if (cs.num_inputs + cs.num_aux >= ShapeAssembly::AUX_BIT)   // columns are 32-bit on the device (csrc/r1cs.hip)
    throw std::invalid_argument("R1CS capture: more than 2^31 variables");
  cs.finish();
}
// host-only self check (bh_test_capture_check): the captured matrices times the assignment a ProvingAssignment
// computes for the same circuit must give that assignment's a, b, c rows.  out4 = [constraints, terms, coefficients in
// the table, rows that differ]; returns the capture time in ms.
double capture_check_for_tests(Circuit &shape_of, Circuit &proved, size_t out4[4]) {
  const double t0 = now_ms();
  ShapeAssembly cs;
  capture_shape(shape_of, cs);
  const double ms = now_ms() - t0;
  ProvingAssignment pa;
  synthesize_assignment(proved, pa);
  const size_t rows = cs.row_ptr[0].size() - 1;
  size_t bad = (rows != pa.a.size() || cs.num_inputs != pa.input_assignment.size() || cs.num_aux != pa.aux_assignment.size()) ? 1 : 0;
  const std::vector<Fr> *want[3] = {&pa.a, &pa.b, &pa.c};
  for (int m = 0; m < 3 && !bad; m++) {
    for (size_t r = 0; r < rows; r++) {
      Fr acc = Fr::zero();
      for (uint32_t t = cs.row_ptr[m][r]; t < cs.row_ptr[m][r + 1]; t++) {
        const uint32_t col = cs.var[m][t];   // (after finish: inputs first, then aux)
        const Fr &v = col < cs.num_inputs ? pa.input_assignment[col] : pa.aux_assignment[col - cs.num_inputs];
        acc = acc + cs.coeffs[cs.coeff[m][t]] * v;
      }
      if (!(acc == (*want[m])[r])) bad++;
    }
  }
  out4[0] = rows; out4[1] = cs.var[0].size() + cs.var[1].size() + cs.var[2].size(); out4[2] = cs.coeffs.size(); out4[3] = bad;
  return ms;
}

R1cs::R1cs(Circuit &shape_of, bh_ctx *ctx) : ctx(ctx) {
  ShapeAssembly cs;
  capture_shape(shape_of, cs);
  num_inputs = cs.num_inputs; num_aux = cs.num_aux; num_constraints = cs.row_ptr[0].size() - 1;
  bh_csr abc[3];
  for (int m = 0; m < 3; m++) abc[m] = bh_csr{cs.row_ptr[m].data(), cs.var[m].data(), cs.coeff[m].data()};
  check(bh_r1cs_create(ctx, num_inputs, num_aux, num_constraints, abc, cs.coeffs.data(), cs.coeffs.size(), &handle));
}
R1cs::R1cs(bh_r1cs *existing, bh_ctx *ctx) : handle(existing), ctx(ctx) {
  check(bh_r1cs_shape(existing, &num_inputs, &num_aux, &num_constraints));
}
std::vector<uint32_t> R1cs::which_is_unsatisfied(const WitnessView *witnesses, size_t k) const {
  return check_witnesses(ctx, *this, witnesses, k, BATCH_WORKSPACE_BYTES);
}
R1cs::~R1cs() { bh_r1cs_release(handle); }

Solver::Solver(const R1cs &r1cs, const bh_solver_desc &desc) : ctx(r1cs.ctx) {
  if (!ctx) throw std::invalid_argument("Solver: the R1cs handle was adopted without its context");
  uint32_t bad = 0xFFFFFFFFu;
  const int rc = bh_r1cs_solver_create(ctx, r1cs.handle, &desc, &bad, &handle);
  if (rc == BH_ERR_INVALID_ARG)
    throw std::invalid_argument(bad == 0xFFFFFFFFu ? std::string("Solver: malformed description")
                                                   : "Solver: variable " + std::to_string(bad) +
                                                         " is not determined by the supplied variables, the hints and the "
                                                         "constraints in order, or is written by a hint that may not write it");
  if (rc != BH_OK) throw std::runtime_error("bh_r1cs_solver_create failed");
  size_t c[5];
  bh_r1cs_solver_info(handle, c);
  supplied = c[0]; defined = c[1]; hinted = c[2]; levels = c[3]; widest_level = c[4];
}
Solver::~Solver() { bh_r1cs_solver_release(handle); }
void Solver::solve_dev(void *inputs_dev, size_t in_stride, void *aux_dev, size_t aux_stride, size_t k, void *stream) const {
  const int rc = bh_r1cs_solve_many_dev(ctx, handle, inputs_dev, in_stride, aux_dev, aux_stride, k, stream);
  if (rc == BH_ERR_INVALID_ARG) throw std::invalid_argument("Solver::solve_dev: bad layout");
  if (rc != BH_OK) throw std::runtime_error("bh_r1cs_solve_many_dev failed");
}
void Solver::solve(Fr *inputs, Fr *aux, size_t k) const {
  if (bh_r1cs_solve_many(ctx, handle, inputs, aux, k) != BH_OK) throw std::runtime_error("bh_r1cs_solve_many failed");
}

WordWitness::WordWitness(bh_ctx *ctx_, const bh_word_witness_desc &desc)
    : ctx(ctx_), num_inputs(desc.n_inputs), num_aux(desc.n_aux), num_ext(desc.n_ext) {
  uint32_t bad[2] = {0, 0xFFFFFFFFu};
  const int rc = bh_word_witness_create(ctx, &desc, &handle, bad);
  if (rc == BH_ERR_INVALID_ARG)
    throw std::invalid_argument(bad[0] ? "WordWitness: program refused, reason " + std::to_string(bad[0]) + " at index " + std::to_string(bad[1])
                                       : std::string("WordWitness: malformed description"));
  if (rc != BH_OK) throw std::runtime_error("bh_word_witness_create failed");
}
WordWitness::~WordWitness() { bh_word_witness_destroy(handle); }
void WordWitness::generate_dev(const void *ext_dev, size_t ext_stride, void *inputs_dev, size_t in_stride, void *aux_dev,
                               size_t aux_stride, size_t k, void *stream) const {
  const int rc = bh_word_witness_generate_dev(ctx, handle, ext_dev, ext_stride, inputs_dev, in_stride, aux_dev, aux_stride, k, stream);
  if (rc == BH_ERR_INVALID_ARG) throw std::invalid_argument("WordWitness::generate_dev: bad layout");
  if (rc != BH_OK) throw std::runtime_error("bh_word_witness_generate_dev failed");
}

Variable WitnessAssignment::alloc(ValueFn f) {
  aux_assignment.push_back(f());
  return Variable::new_unchecked(Index::Aux, aux_assignment.size() - 1);
}
Variable WitnessAssignment::alloc_input(ValueFn f) {
  input_assignment.push_back(f());
  return Variable::new_unchecked(Index::Input, input_assignment.size() - 1);
}

Proof create_proof(Circuit &circuit, const R1cs &r1cs, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  const double t0 = now_ms();
  Recycled<WitnessAssignment> wr(g_witnesses);
  WitnessAssignment &w = *wr;
  synthesize_witness(circuit, r1cs, w);
  const double t1 = now_ms();
  ProveTimings local;
  Proof p = prove_witness(r1cs, params, w.input_assignment.data(), w.input_assignment.size(), w.aux_assignment.data(),
                          w.aux_assignment.size(), r, s, &local);
  if (tm) {
    *tm = local;
    tm->synthesis_ms = (float)(t1 - t0);
    tm->total_ms = (float)(now_ms() - t0);
  }
  return p;
}

// ---- one caller, proofs back to back (groth16.hpp) ---------------------------------------------------------------
Proof AsyncProof::wait(ProveTimings *tm) {
  if (worker.joinable()) worker.join();
  if (tm) *tm = timings;
  if (error) std::rethrow_exception(error);
  return proof;
}
// The device part of a proof on the job's helper thread: runs `prove`, stores the proof and the timings (with the
// synthesis the caller did before, if any) or the exception for AsyncProof::wait
template <class F>
static void start_worker(AsyncProof *j, float synth_ms, F prove) {
  j->worker = std::thread([j, synth_ms, prove] {
    try {
      ProveTimings local = {0, 0, 0, 0};
      j->proof = prove(&local);
      j->timings = local;
      j->timings.synthesis_ms = synth_ms;
      j->timings.total_ms = local.total_ms + synth_ms;
    } catch (...) {
      j->error = std::current_exception();
    }
  });
}
static Proof prove_held_witness(const AsyncProof &j, const R1cs &r1cs, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  const WitnessAssignment &w = *j.witness;
  return prove_witness(r1cs, params, w.input_assignment.data(), w.input_assignment.size(), w.aux_assignment.data(),
                       w.aux_assignment.size(), r, s, tm);
}
std::unique_ptr<AsyncProof> create_proof_async(Circuit &circuit, const R1cs *r1cs, Parameters &params, const Fr &r, const Fr &s) {
  std::unique_ptr<AsyncProof> job(new AsyncProof());
  const double t0 = now_ms();
  if (r1cs) {
    job->witness = g_witnesses.get();
    synthesize_witness(circuit, *r1cs, *job->witness);
  } else {
    job->assignment = g_assignments.get();
    synthesize_assignment(circuit, *job->assignment);
  }
  const float synth_ms = (float)(now_ms() - t0);
  AsyncProof *j = job.get();
  Parameters *pp = &params;
  if (r1cs) start_worker(j, synth_ms, [j, r1cs, pp, r, s](ProveTimings *tm) { return prove_held_witness(*j, *r1cs, *pp, r, s, tm); });
  else start_worker(j, synth_ms, [j, pp, r, s](ProveTimings *tm) { return prove_assignment(*j->assignment, *pp, r, s, tm); });
  return job;
}
std::unique_ptr<AsyncProof> prove_assignment_async(const AssignmentView &v, Parameters &params, const Fr &r, const Fr &s) {
  std::unique_ptr<AsyncProof> job(new AsyncProof());
  Parameters *pp = &params;
  start_worker(job.get(), 0, [v, pp, r, s](ProveTimings *tm) { return prove_assignment(v, *pp, r, s, tm); });
  return job;
}
std::unique_ptr<AsyncProof> prove_witness_async(const R1cs &r1cs, Parameters &params, const void *input_assignment, size_t n_inputs,
                                                const void *aux_assignment, size_t n_aux, const Fr &r, const Fr &s) {
  std::unique_ptr<AsyncProof> job(new AsyncProof());
  job->witness = g_witnesses.get();
  WitnessAssignment &w = *job->witness;
  w.input_assignment.resize(n_inputs);
  w.aux_assignment.resize(n_aux);
  if (n_inputs) memcpy((void *)w.input_assignment.data(), input_assignment, n_inputs * sizeof(Fr));
  if (n_aux) memcpy((void *)w.aux_assignment.data(), aux_assignment, n_aux * sizeof(Fr));
  AsyncProof *j = job.get();
  const R1cs *rp = &r1cs;
  Parameters *pp = &params;
  start_worker(j, 0, [j, rp, pp, r, s](ProveTimings *tm) { return prove_held_witness(*j, *rp, *pp, r, s, tm); });
  return job;
}
void ProofPipeline::retire_oldest() {
  std::unique_ptr<AsyncProof> j = std::move(inflight_.front());
  inflight_.pop_front();
  Done d;
  d.tm = ProveTimings{0, 0, 0, 0};
  try { d.proof = j->wait(&d.tm); } catch (...) { d.error = std::current_exception(); }
  done_.push_back(std::move(d));
}
void ProofPipeline::submit(Circuit &circuit, const Fr &r, const Fr &s) {
  while (inflight_.size() >= depth_) retire_oldest();
  inflight_.push_back(create_proof_async(circuit, r1cs_, params_, r, s));   // synthesis runs here, beside the proofs in flight
}
Proof ProofPipeline::next(ProveTimings *tm) {
  if (done_.empty()) {
    if (inflight_.empty()) throw std::logic_error("ProofPipeline::next without a submitted proof");
    retire_oldest();
  }
  Done d = std::move(done_.front());
  done_.pop_front();
  if (tm) *tm = d.tm;
  if (d.error) std::rethrow_exception(d.error);
  return d.proof;
}

// ---- prover.rs:182-215 ----------------------------------------------------------------------------
Proof create_proof(Circuit &circuit, Parameters &params, const Fr &r, const Fr &s, ProveTimings *tm) {
  const double t0 = now_ms();
  Recycled<ProvingAssignment> pr(g_assignments);
  ProvingAssignment &prover = *pr;
  synthesize_assignment(circuit, prover);
  const double t1 = now_ms();
  BH_TRACE("synthesised: %zu constraints", prover.a.size());
  ProveTimings local;
  Proof p = prove_assignment(prover, params, r, s, &local);
  if (tm) {
    *tm = local;
    tm->synthesis_ms = (float)(t1 - t0);
    tm->total_ms = (float)(now_ms() - t0);
  }
  return p;
}

}  // namespace groth16
