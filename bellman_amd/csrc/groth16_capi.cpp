// The extern "C" entry points of the groth16 layer (declared in include/bellman_hip.h).  The built-in demo circuits and
// their entry points live in the test library (demo_circuits.cpp, include/bellman_hip_test.h).
#include <string.h>

#include <memory>

#include <chrono>
#include <functional>
#include <vector>

#include "groth16_internal.hpp"


// ---------------------------------------------------------------------------------------------------
// C entry points (declared in include/bellman_hip.h)
// ---------------------------------------------------------------------------------------------------
extern "C" {

int bh_groth16_params_create(bh_ctx *ctx, const void *alpha_g1, const void *beta_g1, const void *beta_g2,
                             const void *delta_g1, const void *delta_g2, const void *h, size_t nh, const void *l,
                             size_t nl, const void *a, size_t na, const void *b_g1, size_t nb1, const void *b_g2,
                             size_t nb2, bh_params **out) {
  return guarded([&] {
    groth16::VerifyingKey vk;
    memcpy(&vk.alpha_g1, alpha_g1, 96); memcpy(&vk.beta_g1, beta_g1, 96); memcpy(&vk.beta_g2, beta_g2, 192);
    memcpy(&vk.delta_g1, delta_g1, 96); memcpy(&vk.delta_g2, delta_g2, 192);
    *out = new bh_params{new groth16::Parameters(ctx, vk, (const groth16::G1Affine *)h, nh, (const groth16::G1Affine *)l, nl,
                                                 (const groth16::G1Affine *)a, na, (const groth16::G1Affine *)b_g1, nb1,
                                                 (const groth16::G2Affine *)b_g2, nb2)};
    return BH_OK;
  });
}
int bh_groth16_params_read(bh_ctx *ctx, const void *bytes, size_t len, int checked, bh_params **out) {
  if (!ctx || !out || (len && !bytes)) return BH_ERR_INVALID_ARG;
  return guarded([&] {
    *out = new bh_params{new groth16::Parameters(ctx, bytes, len, checked != 0)};
    return BH_OK;
  });
}
int bh_groth16_generate(bh_ctx *ctx, bh_r1cs *r1cs, const void *g1, const void *g2, const void *alpha, const void *beta,
                        const void *gamma, const void *delta, const void *tau, bh_params **out) {
  if (!ctx || !r1cs || !out) return BH_ERR_INVALID_ARG;
  using namespace groth16;
  return guarded([&] {
    R1csView view(r1cs);
    G1Affine p1; G2Affine p2;
    memcpy(&p1, g1, 96); memcpy(&p2, g2, 192);
    *out = new bh_params{new Parameters(ctx, view.r, p1, p2, read_fr(alpha), read_fr(beta), read_fr(gamma), read_fr(delta), read_fr(tau))};
    return BH_OK;
  });
}
int bh_groth16_generate_from_powers_of_tau(bh_ctx *ctx, bh_r1cs *r1cs, const bh_powers_of_tau *t, bh_params **out) {
  if (!ctx || !r1cs || !t || !out || !t->beta_g2) return BH_ERR_INVALID_ARG;
  using namespace groth16;
  return guarded([&] {
    R1csView view(r1cs);
    PowersOfTau pt;
    pt.tau_g1 = t->tau_g1; pt.tau_g2 = t->tau_g2; pt.alpha_tau_g1 = t->alpha_tau_g1; pt.beta_tau_g1 = t->beta_tau_g1;
    memcpy(&pt.beta_g2, t->beta_g2, 192);
    *out = new bh_params{new Parameters(ctx, view.r, pt)};
    return BH_OK;
  });
}
int bh_groth16_params_rescale_delta(const bh_params *p, const void *d_mont, bh_params **out) {
  if (!p || !d_mont || !out) return BH_ERR_INVALID_ARG;
  return guarded([&] {
    *out = new bh_params{p->p->rescale_delta(read_fr(d_mont)).release()};
    return BH_OK;
  });
}
int bh_groth16_params_write(const bh_params *p, void *buf, size_t cap, size_t *len) {
  if (!p || !len) return BH_ERR_INVALID_ARG;
  return guarded([&] {
    const groth16::Parameters &P = *p->p;
    const size_t need = P.serialized_size();
    *len = need;
    if (!buf || cap < need) return buf ? BH_ERR_INVALID_ARG : BH_OK;   // size query when buf == NULL
    P.write_into((unsigned char *)buf, cap);
    return BH_OK;
  });
}
// prepare_verifying_key (groth16/src/verifier.rs:11-21) on the verifying key of params that carry gamma_g2 and ic
int bh_groth16_pvk_from_params(const bh_params *p, bh_pvk **out) {
  if (!p || !out) return BH_ERR_INVALID_ARG;
  const groth16::Parameters &P = *p->p;
  if (P.vk.ic.empty()) return BH_ERR_INVALID_ARG;
  return bh_groth16_prepare_verifying_key(P.ctx, &P.vk.alpha_g1, &P.vk.beta_g2, &P.vk.gamma_g2, &P.vk.delta_g2, P.vk.ic.data(),
                                          P.vk.ic.size(), out);
}
int bh_groth16_params_vk_ext(const bh_params *p, void *gamma_g2, void *ic_out, size_t ic_cap, size_t *n_ic) {
  if (!p) return BH_ERR_INVALID_ARG;
  const groth16::VerifyingKey &vk = p->p->vk;
  if (gamma_g2) memcpy(gamma_g2, &vk.gamma_g2, 192);
  if (n_ic) *n_ic = vk.ic.size();
  if (ic_out) {
    if (ic_cap < vk.ic.size()) return BH_ERR_INVALID_ARG;
    if (!vk.ic.empty()) memcpy(ic_out, vk.ic.data(), vk.ic.size() * 96);
  }
  return BH_OK;
}
int bh_groth16_params_query(const bh_params *p, int which, const bh_bases **bases, size_t *len) {
  if (!p || which < 0 || which > 4) return BH_ERR_INVALID_ARG;
  const bh_bases *q[5] = {p->p->h, p->p->l, p->p->a, p->p->b_g1, p->p->b_g2};
  if (bases) *bases = q[which];
  if (len) *len = bh_bases_len(q[which]);
  return BH_OK;
}
int bh_groth16_params_vk(const bh_params *p, void *alpha_g1, void *beta_g1, void *beta_g2, void *delta_g1, void *delta_g2) {
  if (!p) return BH_ERR_INVALID_ARG;
  const groth16::VerifyingKey &vk = p->p->vk;
  if (alpha_g1) memcpy(alpha_g1, &vk.alpha_g1, 96);
  if (beta_g1) memcpy(beta_g1, &vk.beta_g1, 96);
  if (beta_g2) memcpy(beta_g2, &vk.beta_g2, 192);
  if (delta_g1) memcpy(delta_g1, &vk.delta_g1, 96);
  if (delta_g2) memcpy(delta_g2, &vk.delta_g2, 192);
  return BH_OK;
}
void bh_proof_write(const void *proof_affine, void *out192) {
  groth16::Proof p;
  memcpy(&p.a, proof_affine, 96);
  memcpy(&p.b, (const char *)proof_affine + 96, 192);
  memcpy(&p.c, (const char *)proof_affine + 288, 96);
  p.write((unsigned char *)out192);
}
void bh_groth16_params_release(bh_params *p) {
  if (!p) return;
  delete p->p;
  delete p;
}

int bh_groth16_prove_assignment(bh_params *params, const void *a_evals, const void *b_evals, const void *c_evals,
                                size_t n_constraints, const void *input_assignment, size_t n_inputs,
                                const void *aux_assignment, size_t n_aux, const uint64_t *a_aux_density,
                                const uint64_t *b_input_density, const uint64_t *b_aux_density, const void *r,
                                const void *s, void *proof_out, float *timings4) {
  using namespace groth16;
  AssignmentView v;
  if (!params || !r || !s || !proof_out ||
      !assignment_view(a_evals, b_evals, c_evals, n_constraints, input_assignment, n_inputs, aux_assignment, n_aux, a_aux_density,
                       b_input_density, b_aux_density, &v))
    return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  // everything that can allocate runs inside the guard
  const int rc = run_guarded([&] { return prove_assignment(v, *params->p, read_fr(r), read_fr(s), &tm); }, proof_out);
  write_timings(timings4, tm);
  return rc;
}

int bh_groth16_prove_witness(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment, size_t n_inputs,
                             const void *aux_assignment, size_t n_aux, const void *r, const void *s, void *proof_out,
                             float *timings4) {
  using namespace groth16;
  if (!params || !r1cs || !r || !s || !proof_out || (n_inputs && !input_assignment) || (n_aux && !aux_assignment))
    return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  const int rc = run_guarded([&] {
    R1csView view(r1cs);
    std::vector<Fr> in(n_inputs), aux(n_aux);   // caller records may be unaligned
    if (n_inputs) memcpy(in.data(), input_assignment, n_inputs * 32);
    if (n_aux) memcpy(aux.data(), aux_assignment, n_aux * 32);
    return prove_witness(view.r, *params->p, in.data(), n_inputs, aux.data(), n_aux, read_fr(r), read_fr(s), &tm);
  }, proof_out);
  write_timings(timings4, tm);
  return rc;
}

int bh_groth16_prove_witness_batch(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs, const void *aux,
                                   size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out, int32_t *rcs,
                                   float *timings4) {
  return prove_witness_batch_guarded(params, r1cs, inputs, n_inputs, aux, n_aux, k, r, s, proofs_out, rcs, timings4, 0);
}

int bh_groth16_prove_witness_batch_checked(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                           const void *aux, size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out,
                                           int32_t *rcs, uint32_t *first_unsatisfied, float *timings4) {
  return prove_witness_batch_guarded(params, r1cs, inputs, n_inputs, aux, n_aux, k, r, s, proofs_out, rcs, timings4, 0,
                                     groth16::BATCH_AUTO, true, first_unsatisfied);
}

int bh_groth16_prove_witness_batch_dev(bh_params *params, const bh_r1cs *r1cs, const void *inputs_dev, size_t in_stride,
                                       const void *aux_dev, size_t aux_stride, size_t k, const void *r, const void *s,
                                       unsigned flags, void *stream, void *proofs_out, int32_t *rcs,
                                       uint32_t *first_unsatisfied, float *timings4) {
  return prove_witness_batch_dev_guarded(params, r1cs, inputs_dev, in_stride, aux_dev, aux_stride, k, r, s, flags, stream,
                                         proofs_out, rcs, first_unsatisfied, timings4);
}

// ---- asynchronous proofs: the device part of a proof on a helper thread (groth16.hpp AsyncProof) ----------------------
int bh_groth16_prove_assignment_async(bh_params *params, const void *a_evals, const void *b_evals, const void *c_evals,
                                      size_t n_constraints, const void *input_assignment, size_t n_inputs,
                                      const void *aux_assignment, size_t n_aux, const uint64_t *a_aux_density,
                                      const uint64_t *b_input_density, const uint64_t *b_aux_density, const void *r,
                                      const void *s, bh_proof_job **out) {
  using namespace groth16;
  AssignmentView v;
  if (!params || !r || !s || !out ||
      !assignment_view(a_evals, b_evals, c_evals, n_constraints, input_assignment, n_inputs, aux_assignment, n_aux, a_aux_density,
                       b_input_density, b_aux_density, &v))
    return BH_ERR_INVALID_ARG;
  return guarded([&] {
    std::unique_ptr<bh_proof_job> pj(new bh_proof_job());
    pj->job = prove_assignment_async(v, *params->p, read_fr(r), read_fr(s));
    *out = pj.release();
    return BH_OK;
  });
}
int bh_groth16_prove_witness_async(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment, size_t n_inputs,
                                   const void *aux_assignment, size_t n_aux, const void *r, const void *s, bh_proof_job **out) {
  using namespace groth16;
  if (!params || !r1cs || !r || !s || !out || (n_inputs && !input_assignment) || (n_aux && !aux_assignment))
    return BH_ERR_INVALID_ARG;
  return guarded([&] {
    std::unique_ptr<bh_proof_job> pj(new bh_proof_job());
    pj->view.reset(new R1csView(r1cs));
    pj->job = prove_witness_async(pj->view->r, *params->p, input_assignment, n_inputs, aux_assignment, n_aux, read_fr(r), read_fr(s));
    *out = pj.release();
    return BH_OK;
  });
}
int bh_groth16_proof_wait(bh_proof_job *job, void *proof_out, float *timings4) {
  using namespace groth16;
  if (!job || !proof_out) return BH_ERR_INVALID_ARG;
  std::unique_ptr<bh_proof_job> pj(job);
  ProveTimings tm = {0, 0, 0, 0};
  const int rc = run_guarded([&] { return pj->job->wait(&tm); }, proof_out);
  write_timings(timings4, tm);
  return rc;
}

int bh_groth16_prove_witness_part(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment, size_t n_inputs,
                                  const void *aux_assignment, size_t n_aux, size_t part, size_t parts, void *sums_out,
                                  float *timings4) {
  using namespace groth16;
  if (!params || !r1cs || !sums_out || (n_inputs && !input_assignment) || (n_aux && !aux_assignment)) return BH_ERR_INVALID_ARG;
  ProveTimings tm = {0, 0, 0, 0};
  const int rc = run_guarded_sums([&] {
    R1csView view(r1cs);
    std::vector<Fr> in(n_inputs), aux(n_aux);
    if (n_inputs) memcpy(in.data(), input_assignment, n_inputs * 32);
    if (n_aux) memcpy(aux.data(), aux_assignment, n_aux * 32);
    return prove_witness_part(view.r, *params->p, in.data(), n_inputs, aux.data(), n_aux, part, parts, &tm);
  }, sums_out);
  write_timings(timings4, tm);
  return rc;
}

void bh_groth16_sums_add(void *acc, const void *other) {
  groth16::MsmSums a, b;
  memcpy(&a, acc, sizeof a);
  memcpy(&b, other, sizeof b);
  a.add(b);
  memcpy(acc, &a, sizeof a);
}

int bh_groth16_assemble(bh_params *params, const void *sums, const void *r, const void *s, void *proof_out) {
  using namespace groth16;
  if (!params || !sums || !r || !s || !proof_out) return BH_ERR_INVALID_ARG;
  MsmSums m;
  memcpy(&m, sums, sizeof m);
  return run_guarded([&] { return assemble_proof(*params->p, m, read_fr(r), read_fr(s)); }, proof_out);
}

int bh_groth16_assemble_many(bh_params *params, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                             int32_t *rcs) {
  using namespace groth16;
  if (!params) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!sums || !r || !s || !proofs_out || !rcs) return BH_ERR_INVALID_ARG;
  return guarded([&] {
    const Parameters &P = *params->p;
    if (P.vk.delta_g1.is_identity() || P.vk.delta_g2.is_identity()) {   // prover.rs:320-324: every proof; nothing is launched
      memset(proofs_out, 0, k * 384);
      for (size_t j = 0; j < k; j++) rcs[j] = BH_ERR_UNEXPECTED_IDENTITY;
      return BH_OK;
    }
    std::vector<MsmSums> m(k);   // caller records may be unaligned
    std::vector<Fr> rr(k), ss(k);
    memcpy(m.data(), sums, k * sizeof(MsmSums));
    memcpy(rr.data(), r, k * 32);
    memcpy(ss.data(), s, k * 32);
    const std::vector<Proof> proofs = assemble_proofs(P, m.data(), rr.data(), ss.data(), k);
    for (size_t j = 0; j < k; j++) {
      write_proof((char *)proofs_out + j * 384, proofs[j]);
      rcs[j] = BH_OK;
    }
    return BH_OK;
  });
}

}  // extern "C"

