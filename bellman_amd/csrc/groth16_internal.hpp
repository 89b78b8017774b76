// Internals shared by the groth16_*.cpp translation units (not part of the public mirror, groth16.hpp).
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <functional>
#include <memory>
#include <stdexcept>
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

}  // namespace detail
void proof_slice_for_tests(size_t n, size_t part, size_t parts, size_t *lo, size_t *hi);   // groth16_prover.cpp
double capture_check_for_tests(bellman::Circuit &shape_of, bellman::Circuit &proved, size_t out4[4]);   // groth16_prover.cpp
}  // namespace groth16

// ---- pieces shared by the C entry points of the product (groth16_capi.cpp) and of the test library (demo_circuits.cpp)
struct bh_params {
  groth16::Parameters *p;
};

inline int run_guarded_sums(const std::function<groth16::MsmSums()> &f, void *sums_out) {
  try {
    groth16::MsmSums m = f();
    memcpy(sums_out, &m, sizeof m);
    return BH_OK;
  } catch (const bellman::SynthesisError &e) { return e.code;
  } catch (const std::invalid_argument &) { return BH_ERR_INVALID_ARG;
  } catch (...) { return BH_ERR_HIP; }
}

// a non-owning groth16::R1cs over a handle that belongs to the C caller
struct R1csView {
  groth16::R1cs r;
  explicit R1csView(const bh_r1cs *h) : r(const_cast<bh_r1cs *>(h)) {}
  ~R1csView() { r.handle = nullptr; }
};

inline int run_guarded(const std::function<groth16::Proof()> &f, void *proof_out) {
  try {
    groth16::Proof p = f();
    memcpy(proof_out, &p.a, 96);
    memcpy((char *)proof_out + 96, &p.b, 192);
    memcpy((char *)proof_out + 288, &p.c, 96);
    return BH_OK;
  } catch (const bellman::SynthesisError &e) { return e.code;
  } catch (const std::invalid_argument &) { return BH_ERR_INVALID_ARG;
  } catch (...) { return BH_ERR_HIP; }
}

// bh_groth16_prove_witness_batch (and _checked), and the test library's twin with a workspace budget of its own (0: the default)
inline int prove_witness_batch_guarded(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs, const void *aux,
                                       size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out, int32_t *rcs,
                                       float *timings4, size_t workspace_budget, int mode = groth16::BATCH_AUTO,
                                       bool checked = false, uint32_t *first_unsatisfied = nullptr) {
  using namespace groth16;
  if (!params || !r1cs) return BH_ERR_INVALID_ARG;
  if (k && (!r || !s || !proofs_out || !rcs || (n_inputs && !inputs) || (n_aux && !aux))) return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  int rc = BH_OK;
  try {
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
    for (size_t j = 0; j < k; j++) {
      char *out = (char *)proofs_out + j * 384;
      rcs[j] = codes[j];
      if (codes[j] == BH_OK) { memcpy(out, &proofs[j].a, 96); memcpy(out + 96, &proofs[j].b, 192); memcpy(out + 288, &proofs[j].c, 96); }
      else memset(out, 0, 384);
    }
  } catch (const bellman::SynthesisError &e) { rc = e.code;
  } catch (const std::invalid_argument &) { rc = BH_ERR_INVALID_ARG;
  } catch (...) { rc = BH_ERR_HIP; }
  if (timings4) { timings4[0] = tm.synthesis_ms; timings4[1] = tm.h_poly_ms; timings4[2] = tm.msm_ms; timings4[3] = tm.total_ms; }
  return rc;
}

struct bh_proof_job {
  // members are destroyed in reverse order: the job (whose destructor joins the helper thread) before the view of the
  // constraint matrices that thread reads
  std::unique_ptr<R1csView> view;
  std::unique_ptr<groth16::AsyncProof> job;
  int early_rc = BH_OK;
};
