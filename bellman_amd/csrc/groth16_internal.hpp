// Internals shared by the groth16_*.cpp translation units (not part of the public mirror, groth16.hpp).
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>
#include <string.h>

#include "env_settings.hpp"
#include "groth16.hpp"

#define BH_TRACE(...) do { if (bh::env().debug) { fprintf(stderr, "[groth16 %.2f ms] ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count()); fprintf(stderr, __VA_ARGS__); fputc(10, stderr); fflush(stderr); } } while (0)

namespace groth16 {
namespace detail {

// C-ABI return code -> the exception the mirror throws (src/lib.rs:303-319); HIP failures are never
// turned into a CPU path
inline void check(int rc) {
  switch (rc) {
    case BH_OK: return;
    case BH_ERR_UNEXPECTED_IDENTITY: throw bellman::SynthesisError(rc, "UnexpectedIdentity");
    case BH_ERR_UNEXPECTED_EOF: throw bellman::SynthesisError(rc, "IoError(UnexpectedEof): expected more bases from source");
    case BH_ERR_DEGREE_TOO_LARGE: throw bellman::SynthesisError(rc, "PolynomialDegreeTooLarge");
    case BH_ERR_UNSATISFIABLE: throw bellman::SynthesisError(rc, "Unsatisfiable");
    default: throw std::runtime_error("bellman_hip: HIP/runtime failure (no CPU fallback)");
  }
}

struct DevBuf {   // a device buffer from the context's pool, returned on scope exit
  bh_ctx *ctx;
  void *p = nullptr;
  DevBuf(bh_ctx *c, size_t bytes) : ctx(c) { check(bh_dev_alloc(ctx, bytes, &p)); }
  ~DevBuf() { if (p) bh_dev_free(ctx, p); }
  DevBuf(const DevBuf &) = delete;
};

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the eight multiexps of a proof (prover.rs:217-360), stated once for every prover path --------------------------
// Slots in the order the reference waits for them (prover.rs:339-354): a_inputs, a_aux, b_g1_inputs, b_g1_aux,
// b_g2_inputs, b_g2_aux, h, l.  It is MsmSums' field order too.
enum Slot { A_IN, A_AUX, B1_IN, B1_AUX, B2_IN, B2_AUX, H, L, N_SLOTS };
constexpr Slot WAIT_ORDER[N_SLOTS] = {A_IN, A_AUX, B1_IN, B1_AUX, B2_IN, B2_AUX, H, L};
inline size_t slot_bytes(int slot) { return slot == B2_IN || slot == B2_AUX ? sizeof(G2Affine) : sizeof(G1Affine); }
inline void *sum_at(MsmSums &m, int slot) {
  void *field[N_SLOTS] = {&m.a_in, &m.a_aux, &m.b1_in, &m.b1_aux, &m.b2_in, &m.b2_aux, &m.h, &m.l};
  return field[slot];
}
// The order the seven multiexps that need only the assignments are issued in; H is placed by the path (it needs the h
// block).  Issue order = order of the bucket accumulations on the device (the accumulation chain, common.hpp): the G2
// multiexp first - the longest job, its reduction tail then runs beside the G1 accumulations
// (profiles/archive/r3_call2_proof_timeline.txt, r3_call4_proof_timeline.txt).  For a small proof the host needs ~0.2 ms to
// enqueue each job's ~20 launches, so what is issued last finishes last: G2 first there too
// (profiles/archive/r2_call21_mimc_timeline.txt).  The order of waits is the reference's whatever the order of issue.
constexpr Slot ISSUE_ORDER[7] = {B2_AUX, L, A_IN, A_AUX, B1_IN, B1_AUX, B2_IN};
// the order of the UNCHANGED call sites of prover.rs:244-318 (the call-site transcriptions of the unpatched prover)
constexpr Slot REFERENCE_ORDER[N_SLOTS] = {H, L, A_IN, A_AUX, B1_IN, B1_AUX, B2_IN, B2_AUX};

enum ScalarSource { FROM_INPUTS, FROM_AUX, FROM_QUOTIENT };
enum { DENSITY_FULL = -1, DENSITY_A_AUX = 0, DENSITY_B_INPUT = 1, DENSITY_B_AUX = 2 };   // bh_r1cs_density's `which`
struct Query {
  bh_bases *bases;
  size_t skip;            // bases the query starts at (before what a slice's skipped scalars consume)
  ScalarSource scalars;
  int density;
};
struct QueryTable {
  Query q[N_SLOTS];
  const Query &operator[](int slot) const { return q[slot]; }
};
inline QueryTable queries(const Parameters &p, size_t n_in, size_t b_in_total) {
  QueryTable t;
  // get_a(num_inputs, _) -> ((a,0),(a,num_inputs))            groth16/src/lib.rs:451-457
  t.q[A_IN] = Query{p.a, 0, FROM_INPUTS, DENSITY_FULL};
  t.q[A_AUX] = Query{p.a, n_in, FROM_AUX, DENSITY_A_AUX};
  // get_b_g1/g2(b_input_density_total, _) -> ((b,0),(b,total))   groth16/src/lib.rs:459-473
  t.q[B1_IN] = Query{p.b_g1, 0, FROM_INPUTS, DENSITY_B_INPUT};
  t.q[B1_AUX] = Query{p.b_g1, b_in_total, FROM_AUX, DENSITY_B_AUX};
  t.q[B2_IN] = Query{p.b_g2, 0, FROM_INPUTS, DENSITY_B_INPUT};
  t.q[B2_AUX] = Query{p.b_g2, b_in_total, FROM_AUX, DENSITY_B_AUX};
  t.q[H] = Query{p.h, 0, FROM_QUOTIENT, DENSITY_FULL};      // a.len() - 1 coefficients, prover.rs:238-244
  t.q[L] = Query{p.l, 0, FROM_AUX, DENSITY_FULL};
  return t;
}

// set bits among the first n of an LSB0 bitmap: get_total_density (multiexp.rs:154-156), and the bases a slice's skipped
// scalars consume
inline size_t popcount_bits(const uint64_t *w, size_t n) {
  size_t t = 0;
  for (size_t i = 0; i < n / 64; i++) t += (size_t)__builtin_popcountll(w[i]);
  if (n & 63) t += (size_t)__builtin_popcountll(w[n / 64] & ((uint64_t(1) << (n & 63)) - 1));
  return t;
}
// The three density maps of a proof (prover.rs:59-61), indexed by DENSITY_*: LSB0 words on the device (null where a path
// hands the host words over) and on the host, and b_input_density's total.
struct Densities {
  const uint64_t *dev[3] = {nullptr, nullptr, nullptr}, *host[3] = {nullptr, nullptr, nullptr};
  size_t b_in_total = 0;
  std::unique_ptr<DevBuf> uploaded[3];   // the device copies `upload` made (released with this object)
  const uint64_t *dev_of(int density) const { return density < 0 ? nullptr : dev[density]; }
  const uint64_t *host_of(int density) const { return density < 0 ? nullptr : host[density]; }
  void on_host(const uint64_t *a_aux, const uint64_t *b_input, const uint64_t *b_aux, size_t n_in) {
    host[DENSITY_A_AUX] = a_aux; host[DENSITY_B_INPUT] = b_input; host[DENSITY_B_AUX] = b_aux;
    b_in_total = popcount_bits(b_input, n_in);
  }
  void upload(bh_ctx *ctx, size_t n_in, size_t n_aux, void *stream) {   // after on_host
    const size_t bits[3] = {n_aux, n_in, n_aux};
    try {
      for (int i = 0; i < 3; i++) {
        const size_t nw = (bits[i] + 63) / 64;
        uploaded[i].reset(new DevBuf(ctx, nw * 8 + 8));
        if (nw) check(bh_dev_upload_on(ctx, uploaded[i]->p, host[i], nw * 8, stream));
        dev[i] = (const uint64_t *)uploaded[i]->p;
      }
    } catch (...) {
      // the maps uploaded so far are released as the caller's frame unwinds: not under their queued uploads.  (The caller
      // synchronises `stream` once everything is queued; from then on only multiexp jobs read the maps.)
      (void)bh_stream_synchronize(ctx, stream);
      throw;
    }
  }
  void of(const R1cs &r1cs) {   // resident with the matrices
    for (int i = 0; i < 3; i++) check(bh_r1cs_density(r1cs.handle, i, &dev[i], &host[i], i == DENSITY_B_INPUT ? &b_in_total : nullptr));
  }
};

// EvaluationDomain::from_coeffs (domain.rs:47-79): the smallest power of two >= n_constraints
struct Domain { size_t m; uint32_t log_m; };
inline Domain domain_of(size_t n_constraints) {
  Domain d{1, 0};
  while (d.m < n_constraints) {
    d.m *= 2;
    d.log_m++;
    if (d.log_m >= 32) throw bellman::SynthesisError(BH_ERR_DEGREE_TOO_LARGE, "PolynomialDegreeTooLarge");
  }
  return d;
}

// the subversion check of prover.rs:320-324: an identity delta is refused by every path that finishes a proof
inline bool subverted(const Parameters &p) { return p.vk.delta_g1.is_identity() || p.vk.delta_g2.is_identity(); }
// An `inputs` multiexp of at most this many terms is handed over with its host scalars: the library answers it on the
// host instead of running a kernel pipeline per term
constexpr size_t HOST_INPUTS_MAX = 8;

// What a proof reports, from the codes of its eight waits (in slot order).  prover.rs:320-324 returns UnexpectedIdentity
// for an identity delta BEFORE any multiexp is waited on: it beats whatever a multiexp reports (e.g. UnexpectedEof from a
// short query); then the first failing `?` in wait order.  A negative code is a runtime failure: the call's, not a proof's.
inline int first_failure(const Parameters &p, const int codes[N_SLOTS]) {
  if (subverted(p)) return BH_ERR_UNEXPECTED_IDENTITY;
  for (Slot s : WAIT_ORDER)
    if (codes[s] != BH_OK) return codes[s];
  return BH_OK;
}

// Every issued multiexp owns device buffers and reads the caller's: each is waited on exactly once, even when something
// throws between issue and wait (the Rust MsmJob's Drop).  Declare it AFTER every buffer a job reads - it is then
// destroyed first and drains whatever is still in flight before those buffers are released.
inline void drain(bh_msm_job *j) { unsigned char sink[192]; (void)bh_msm_wait(j, sink); }
inline void drain(bh_msm_many_job *j) { (void)bh_msm_many_wait(j, nullptr, nullptr, nullptr, nullptr); }
template <class Job>
struct InFlight {
  std::vector<Job *> at;   // issue into &at[i]; null: not issued, or taken
  explicit InFlight(size_t n) : at(n, nullptr) {}
  InFlight(const InFlight &) = delete;
  Job *take(size_t i) { Job *j = at[i]; at[i] = nullptr; return j; }
  ~InFlight() { for (Job *&j : at) if (j) { drain(j); j = nullptr; } }
};
// the eight waits of prover.rs:339-354 on jobs held by slot, then the verdict: every job is waited on (it owns device
// resources), even when an earlier one fails
inline void wait_eight(InFlight<bh_msm_job> &jobs, const Parameters &p, MsmSums &out) {
  int codes[N_SLOTS];
  for (Slot s : WAIT_ORDER) codes[s] = bh_msm_wait(jobs.take(s), sum_at(out, s));
  BH_TRACE("waits done rc=%d %d %d %d %d %d %d %d", codes[0], codes[1], codes[2], codes[3], codes[4], codes[5], codes[6], codes[7]);
  check(first_failure(p, codes));
}

// ---- what the k-proof paths (groth16_batch.cpp) share with the single proof: defined in groth16_prover.cpp -------------
struct ProofStream {   // uploads + h block of one proof; independent of other proofs in flight
  bh_ctx *ctx;
  void *st = nullptr;
  explicit ProofStream(bh_ctx *c);
  ~ProofStream();   // synchronises, then destroys
  ProofStream(const ProofStream &) = delete;
};
// Declared after every DevBuf the proof stream writes (and so destroyed before them): if an exception
// unwinds the frame, queued uploads / memsets / evaluations finish before their targets return to the
// shared pool, where another proof's thread could pick them up.
struct StreamDrain {
  ProofStream &ps;
  ~StreamDrain() { if (ps.st) (void)bh_stream_synchronize(ps.ctx, ps.st); }
};
// What differs between the ways of getting a proof's assignment and constraint evaluations into HBM
struct AssignmentSource {
  const Fr *inputs; size_t n_in;
  const Fr *aux; size_t n_aux;
  size_t n_cons;
  // host path (prove_assignment): evaluations and density bitmaps computed during synthesis - plain views, so that the
  // C entry point hands the caller's arrays through without copying them
  bool host = false;
  const Fr *a = nullptr, *b = nullptr, *c = nullptr;
  const uint64_t *a_aux_density = nullptr, *b_input_density = nullptr, *b_aux_density = nullptr;   // LSB0 words
  // device path (prove_witness): matrices and densities already resident
  const R1cs *r1cs = nullptr;
  // device form of the witness (prove_witness_batch_dev): the two vectors where the caller holds them in device memory,
  // read in place - nothing is uploaded.  `inputs` is then a host copy for the `inputs` multiexps that are answered on the
  // host (n_in <= HOST_INPUTS_MAX), or null; `aux` is null.
  const void *inputs_dev = nullptr, *aux_dev = nullptr;
  bool resident = false;
};
// prover.rs:217-318 + the waits of :339-354: the eight multiexp results (of part `part` of `parts`' slices)
void msm_sums(const AssignmentSource &src, Parameters &params, size_t part, size_t parts, MsmSums &out, ProveTimings *tm);
// prover.rs:320-338: the part of the proof elements that depends on the verifying key and r, s only
struct ProofBlinding {
  G1Affine g_a, g_c;
  G2Affine g_b;
};
// The blinding terms of k (r, s) pairs on min(k, 8) helper threads, started at construction.  They involve only the
// verifying key, r and s (prover.rs:326-338; five scalar multiplications, ~0.9 ms of host arithmetic per proof) and run
// beside the enqueueing of the multiexps and the GPU work: for a small proof they are as long as everything else
// together.  A failure there (identity delta) is kept in `error`, to be reported after the jobs drain.
struct Blinding {
  std::vector<ProofBlinding> terms;
  std::exception_ptr error;
  Blinding(const Parameters &params, const Fr *r, const Fr *s, size_t k);
  void join() { for (std::thread &t : threads_) if (t.joinable()) t.join(); }
  ~Blinding() { join(); }

 private:
  std::mutex mu_;
  std::vector<std::thread> threads_;
};
Proof finish_proof(const ProofBlinding &b, const MsmSums &m, const Fr &r, const Fr &s);   // prover.rs:339-360
// a witness has the shape of the captured circuit, or std::invalid_argument - before anything runs
void require_shape(const R1cs &r1cs, const WitnessView *witnesses, size_t k);
// The witnesses w[0 .. g) into two strided device buffers (strides = the vectors' lengths), on stream st.  With `coalesce`
// and every host vector starting where the one before ends, ONE upload per vector kind; otherwise one per witness.
void upload_witnesses(bh_ctx *ctx, const WitnessView *w, size_t g, void *d_in, void *d_aux, void *st, bool coalesce);
// which_is_unsatisfied for k witnesses: groups whose device copies stay within `budget` bytes, one bh_r1cs_check_many_dev each
std::vector<uint32_t> check_witnesses(bh_ctx *ctx, const R1cs &r1cs, const WitnessView *witnesses, size_t k, size_t budget);

}  // namespace detail
// groth16_prover.cpp: bh_proof_finish_dev with params' verifying key
int finish_proofs_dev(const Parameters &params, const void *sums_dev, const void *r_dev, const void *s_dev, size_t k,
                      void *proofs_dev, void *stream);
void proof_slice_for_tests(size_t n, size_t part, size_t parts, size_t *lo, size_t *hi);   // groth16_prover.cpp
double capture_check_for_tests(bellman::Circuit &shape_of, bellman::Circuit &proved, size_t out4[4]);   // groth16_prover.cpp
// `circuit`'s witness into w (the constant one first, prover.rs:194); groth16_prover.cpp
void synthesize_witness(bellman::Circuit &circuit, const R1cs &r1cs, WitnessAssignment &w);
}  // namespace groth16

// ---- the C boundary: pieces shared by the entry points of the product (groth16_capi.cpp) and of the test library
// (demo_circuits.cpp, groth16_callsites.cpp)
struct bh_params {
  groth16::Parameters *p;
};

// no C++ exception may cross the C boundary: runs body() and answers its return code, or the code of what it threw
template <class F>
int guarded(F &&body) {
  try {
    return body();
  } catch (const bellman::IoError &e) { return e.code;   // (thrown by the read paths only)
  } catch (const bellman::SynthesisError &e) { return e.code;
  } catch (const std::invalid_argument &) { return BH_ERR_INVALID_ARG;
  } catch (...) { return BH_ERR_HIP; }
}
inline void write_proof(void *out384, const groth16::Proof &p) {
  memcpy(out384, &p.a, 96);
  memcpy((char *)out384 + 96, &p.b, 192);
  memcpy((char *)out384 + 288, &p.c, 96);
}
inline void write_timings(float *timings4, const groth16::ProveTimings &tm) {
  if (timings4) { timings4[0] = tm.synthesis_ms; timings4[1] = tm.h_poly_ms; timings4[2] = tm.msm_ms; timings4[3] = tm.total_ms; }
}
inline groth16::Fr read_fr(const void *mont32) {   // caller records may be unaligned
  groth16::Fr f;
  memcpy(&f, mont32, 32);
  return f;
}
template <class F>
int run_guarded_sums(F &&f, void *sums_out) {
  return guarded([&] {
    groth16::MsmSums m = f();
    memcpy(sums_out, &m, sizeof m);
    return BH_OK;
  });
}
template <class F>
int run_guarded(F &&f, void *proof_out) {
  return guarded([&] {
    write_proof(proof_out, f());
    return BH_OK;
  });
}
// The C form of a host-synthesised assignment as a view of the caller's arrays: they are only read as bytes (uploads, the
// tiny input multiexps), never copied.  False for a null array that should hold something.
inline bool assignment_view(const void *a_evals, const void *b_evals, const void *c_evals, size_t n_constraints,
                            const void *input_assignment, size_t n_inputs, const void *aux_assignment, size_t n_aux,
                            const uint64_t *a_aux_density, const uint64_t *b_input_density, const uint64_t *b_aux_density,
                            groth16::AssignmentView *v) {
  using groth16::Fr;
  if ((n_constraints && (!a_evals || !b_evals || !c_evals)) || (n_inputs && (!input_assignment || !b_input_density)) ||
      (n_aux && (!aux_assignment || !a_aux_density || !b_aux_density)))
    return false;
  *v = groth16::AssignmentView{(const Fr *)a_evals, (const Fr *)b_evals, (const Fr *)c_evals, n_constraints,
                               (const Fr *)input_assignment, n_inputs, (const Fr *)aux_assignment, n_aux,
                               a_aux_density, b_input_density, b_aux_density};
  return true;
}

// a non-owning groth16::R1cs over a handle that belongs to the C caller
struct R1csView {
  groth16::R1cs r;
  explicit R1csView(const bh_r1cs *h) : r(const_cast<bh_r1cs *>(h)) {}
  ~R1csView() { r.handle = nullptr; }
};

// bh_groth16_prove_witness_batch (and _checked), and the test library's twins with a workspace budget and a mode of their
// own (0: the default); groth16_batch.cpp
int prove_witness_batch_guarded(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs, const void *aux,
                                size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out, int32_t *rcs,
                                float *timings4, size_t workspace_budget, int mode = groth16::BATCH_AUTO, bool checked = false,
                                uint32_t *first_unsatisfied = nullptr);

// bh_groth16_prove_witness_batch_dev, and the test library's twin with a workspace budget and a mode; groth16_batch.cpp
int prove_witness_batch_dev_guarded(bh_params *params, const bh_r1cs *r1cs, const void *inputs_dev, size_t in_stride,
                                    const void *aux_dev, size_t aux_stride, size_t k, const void *r, const void *s, unsigned flags,
                                    void *stream, void *proofs_out, int32_t *rcs, uint32_t *first_unsatisfied, float *timings4,
                                    size_t workspace_budget = 0, int mode = groth16::BATCH_AUTO);

struct bh_proof_job {
  // members are destroyed in reverse order: the job (whose destructor joins the helper thread) before the view of the
  // constraint matrices that thread reads
  std::unique_ptr<R1csView> view;
  std::unique_ptr<groth16::AsyncProof> job;
  int early_rc = BH_OK;
};
