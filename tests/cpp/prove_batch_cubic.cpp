// A C++ user of groth16::prove_witness_batch in the bellman mirror (bellman_amd/csrc/groth16.hpp): nine witnesses of the
// cubic circuit of prove_cubic.cpp proved in one call - as shipped (proofs in flight), through the grouped path with the
// default workspace budget and with one that fits two witnesses per group - must give exactly the proofs of nine prove_witness calls; a witness of the wrong shape is refused
// before anything runs.  The generators g1 (96 B) | g2 (192 B) come from a file written by tests/test_gpu_prove_batch.py.
// Prints "prove_witness_batch ok" and exits 0 when every expectation holds.
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

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
  try {
    CubicDemo shape;
    shape.x = Fr::zero();
    groth16::R1cs r1cs(shape, ctx);
    groth16::Parameters params(ctx, r1cs, g1, g2, rand_fr(), rand_fr(), rand_fr(), rand_fr(), rand_fr());
    const size_t k = 9;
    std::vector<groth16::WitnessAssignment> ws(k);
    std::vector<groth16::WitnessView> views;
    std::vector<std::pair<Fr, Fr>> rs;
    std::vector<groth16::Proof> want;
    for (size_t j = 0; j < k; j++) {
      CubicDemo c;
      c.x = rand_fr();
      ws[j].alloc_input([] { return Fr::one(); });
      c.synthesize(ws[j]);
      views.push_back(groth16::WitnessView{ws[j].input_assignment.data(), ws[j].input_assignment.size(),
                                           ws[j].aux_assignment.data(), ws[j].aux_assignment.size()});
      rs.emplace_back(rand_fr(), rand_fr());
      want.push_back(groth16::prove_witness(r1cs, params, views[j].inputs, views[j].n_inputs, views[j].aux, views[j].n_aux,
                                            rs[j].first, rs[j].second));
    }
    const std::vector<groth16::Proof> got = groth16::prove_witness_batch(r1cs, params, views, rs);
    const std::vector<groth16::Proof> grouped = groth16::prove_witness_batch(r1cs, params, views, rs, nullptr, 0, groth16::BATCH_GROUPED);
    // (m = 4 for three constraints + two input rows -> 8: a budget of (2 + 3) * 8 * 32 bytes fits two witnesses per group)
    const std::vector<groth16::Proof> cut = groth16::prove_witness_batch(r1cs, params, views, rs, nullptr, (2 + 3) * 8 * 32, groth16::BATCH_GROUPED);
    if (got.size() != k || cut.size() != k || grouped.size() != k) rc = 5;
    for (size_t j = 0; j < k && !rc; j++)
      if (memcmp(&got[j], &want[j], sizeof want[j]) != 0 || memcmp(&cut[j], &want[j], sizeof want[j]) != 0 ||
          memcmp(&grouped[j], &want[j], sizeof want[j]) != 0) {
        fprintf(stderr, "batch proof %zu differs\n", j);
        rc = 6;
      }
    if (!groth16::prove_witness_batch(r1cs, params, {}, {}).empty()) rc = 7;
    std::vector<groth16::WitnessView> bad = views;
    bad[2].n_aux -= 1;
    bool refused = false;
    try { (void)groth16::prove_witness_batch(r1cs, params, bad, rs); } catch (const std::invalid_argument &) { refused = true; }
    if (!refused) rc = 8;
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 10 + e.code;
  }
  bh_ctx_destroy(ctx);
  if (!rc) printf("prove_witness_batch ok\n");
  return rc;
}
