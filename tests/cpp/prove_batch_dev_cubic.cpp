// A C++ user of the device-witness batch prover in the bellman mirror (bellman_amd/csrc/groth16.hpp): four witnesses of the
// cubic circuit of prove_cubic.cpp live in strided device buffers that hold only ONE and x, Solver::solve_dev completes
// them there, and prove_witness_batch_dev (checked; tails on the host and on the device) gives the proofs prove_witness
// gives for the host-synthesised witnesses; assemble_proofs equals assemble_proof; both finish bits are refused.
// The generators g1 (96 B) | g2 (192 B) come from a file written by tests/test_gpu_prove_batch_dev.py.
// Prints "prove_batch_dev ok" and exits 0 when every expectation holds.
#include <stdio.h>
#include <string.h>

#include <stdexcept>
#include <vector>

#include "../../bellman_amd/csrc/groth16.hpp"

using namespace bellman;

struct CubicDemo : Circuit {
  Fr x;
  void synthesize(ConstraintSystem &cs) override {
    const Fr x2v = x * x, x3v = x2v * x, outv = x3v + x + Fr::from_u64(5);
    Variable xv = cs.alloc([&] { return x; });
    Variable x2 = cs.alloc([&] { return x2v; });
    Variable x3 = cs.alloc([&] { return x3v; });
    Variable out = cs.alloc_input([&] { return outv; });
    cs.enforce([&](LinearCombination lc) { return lc + xv; }, [&](LinearCombination lc) { return lc + xv; },
               [&](LinearCombination lc) { return lc + x2; });
    cs.enforce([&](LinearCombination lc) { return lc + x2; }, [&](LinearCombination lc) { return lc + xv; },
               [&](LinearCombination lc) { return lc + x3; });
    cs.enforce([&](LinearCombination lc) { return lc + x3 + xv + std::make_pair(Fr::from_u64(5), ConstraintSystem::one()); },
               [&](LinearCombination lc) { return lc + ConstraintSystem::one(); },
               [&](LinearCombination lc) { return lc + out; });
  }
};

static bool same(const groth16::Proof &a, const groth16::Proof &b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  groth16::G1Affine g1;
  groth16::G2Affine g2;
  if (fread(&g1, 96, 1, f) != 1 || fread(&g2, 192, 1, f) != 1) return 3;
  fclose(f);
  bh_ctx *ctx = nullptr;
  if (bh_ctx_create(0, &ctx) != BH_OK) { fprintf(stderr, "no gfx950 device (no CPU fallback)\n"); return 4; }
  int rc = 0;
  uint64_t state = 0x2545F4914F6CDD1DULL;
  auto rng = [&state] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto rand_fr = [&] { uint64_t w[8]; for (uint64_t &x : w) x = rng(); return Fr::from_u512(w); };
  void *d_in = nullptr, *d_aux = nullptr;
  try {
    CubicDemo shape;
    shape.x = Fr::zero();
    groth16::R1cs r1cs(shape, ctx);
    groth16::Parameters params(ctx, r1cs, g1, g2, rand_fr(), rand_fr(), rand_fr(), rand_fr(), rand_fr());
    const size_t k = 4, ni = r1cs.num_inputs, na = r1cs.num_aux;
    const size_t in_stride = ni * 32 + 32, aux_stride = na * 32 + 64;   // padded: a vector does not start where the last ends
    const uint32_t supplied[1] = {(uint32_t)ni};   // x: the first aux variable
    bh_solver_desc desc;
    memset(&desc, 0, sizeof desc);
    desc.supplied = supplied;
    desc.n_supplied = 1;
    std::unique_ptr<groth16::Solver> solver = r1cs.solver(desc);
    std::vector<Fr> h_in(k * in_stride / 32, Fr::from_u64(77)), h_aux(k * aux_stride / 32, Fr::from_u64(99));
    std::vector<groth16::Proof> want(k);
    std::vector<std::pair<Fr, Fr>> rs;
    for (size_t j = 0; j < k; j++) {
      CubicDemo c;
      c.x = rand_fr();
      groth16::WitnessAssignment w;
      w.alloc_input([] { return Fr::one(); });
      c.synthesize(w);
      rs.emplace_back(rand_fr(), rand_fr());
      want[j] = groth16::prove_witness(r1cs, params, w.input_assignment.data(), ni, w.aux_assignment.data(), na, rs[j].first, rs[j].second);
      h_in[j * in_stride / 32] = Fr::one();
      h_aux[j * aux_stride / 32] = c.x;
    }
    if (bh_dev_alloc(ctx, k * in_stride, &d_in) != BH_OK || bh_dev_alloc(ctx, k * aux_stride, &d_aux) != BH_OK) throw std::runtime_error("alloc");
    if (bh_dev_upload(ctx, d_in, h_in.data(), k * in_stride) != BH_OK || bh_dev_upload(ctx, d_aux, h_aux.data(), k * aux_stride) != BH_OK)
      throw std::runtime_error("upload");
    void *stream = nullptr;
    if (bh_stream_create(ctx, &stream) != BH_OK) throw std::runtime_error("stream");
    solver->solve_dev(d_in, in_stride, d_aux, aux_stride, k, stream);
    const groth16::DeviceWitnesses dw{d_in, in_stride, d_aux, aux_stride, k};
    for (unsigned finish : {BH_PROVE_FINISH_HOST, BH_PROVE_FINISH_DEVICE, 0u}) {
      std::vector<uint32_t> first;
      const std::vector<groth16::Proof> got = groth16::prove_witness_batch_dev(r1cs, params, dw, rs, BH_PROVE_CHECK | finish, stream, &first);
      if (got.size() != k || first != std::vector<uint32_t>(k, BH_R1CS_SATISFIED)) rc = 5;
      for (size_t j = 0; j < k && !rc; j++)
        if (!same(got[j], want[j])) rc = 6;
    }
    bh_stream_destroy(ctx, stream);
    try {
      groth16::prove_witness_batch_dev(r1cs, params, dw, rs, BH_PROVE_FINISH_HOST | BH_PROVE_FINISH_DEVICE);
      rc = 7;
    } catch (const std::invalid_argument &) {
    }
    // assemble_proofs against assemble_proof on the sums of two witnesses
    std::vector<Fr> back_in(k * in_stride / 32), back_aux(k * aux_stride / 32);
    if (bh_dev_download(ctx, back_in.data(), d_in, k * in_stride) != BH_OK || bh_dev_download(ctx, back_aux.data(), d_aux, k * aux_stride) != BH_OK)
      throw std::runtime_error("download");
    if (!(back_in[ni] == Fr::from_u64(77)) || !(back_aux[na] == Fr::from_u64(99))) rc = 8;   // the padding is as it was
    std::vector<groth16::MsmSums> sums;
    std::vector<Fr> r, s;
    for (size_t j = 0; j < 2; j++) {
      sums.push_back(groth16::prove_witness_part(r1cs, params, back_in.data() + j * in_stride / 32, ni, back_aux.data() + j * aux_stride / 32,
                                                 na, 0, 1));
      r.push_back(rs[j].first);
      s.push_back(rs[j].second);
    }
    const std::vector<groth16::Proof> many = groth16::assemble_proofs(params, sums.data(), r.data(), s.data(), 2);
    for (size_t j = 0; j < 2; j++)
      if (!same(many[j], groth16::assemble_proof(params, sums[j], r[j], s[j])) || !same(many[j], want[j])) rc = 9;
  } catch (const std::exception &e) {
    fprintf(stderr, "exception: %s\n", e.what());
    rc = 20;
  }
  if (d_in) bh_dev_free(ctx, d_in);
  if (d_aux) bh_dev_free(ctx, d_aux);
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("prove_batch_dev ok\n");
  return rc;
}
