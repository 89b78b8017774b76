// A C++ user of BatchVerifier::verify_each / find_invalid in the bellman mirror (bellman_amd/csrc/groth16.hpp): twelve
// proofs of the cubic circuit of prove_cubic.cpp, two of them spoiled (a wrong public input; C of another proof); the
// per-proof verdicts must name exactly those two, a clean batch must give none.  The generators g1 (96 B) | g2 (192 B) come
// from a file written by tests/test_gpu_verify_each_cpp.py.  Prints "verify_each ok" and exits 0 when every expectation
// holds.
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

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
  Fr image() const { return x * x * x + x + Fr::from_u64(5); }
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
    std::unique_ptr<groth16::PreparedVerifyingKey> pvk = groth16::prepare_verifying_key(params);
    std::vector<CubicDemo> circuits(12);
    std::vector<groth16::Proof> proofs;
    for (size_t i = 0; i < circuits.size(); i++) {
      circuits[i].x = rand_fr();
      proofs.push_back(groth16::create_random_proof(circuits[i], params, rng));
    }
    groth16::BatchVerifier clean, spoiled;
    for (size_t i = 0; i < circuits.size(); i++) {
      clean.queue(proofs[i], {circuits[i].image()});
      groth16::Proof p = proofs[i];
      Fr in = circuits[i].image();
      if (i == 3) in = in + Fr::from_u64(1);
      if (i == 10) p.c = proofs[4].c;
      spoiled.queue(p, {in});
    }
    const std::vector<int> ok = clean.verify_each(*pvk);
    if (ok.size() != circuits.size()) rc = 5;
    for (int v : ok)
      if (v != BH_OK) rc = 6;
    if (!clean.find_invalid(rng, *pvk).empty()) rc = 7;
    const std::vector<int> v = spoiled.verify_each(*pvk);
    for (size_t i = 0; i < v.size(); i++)
      if (v[i] != ((i == 3 || i == 10) ? BH_ERR_INVALID_PROOF : BH_OK)) rc = 8;
    const std::vector<size_t> bad = spoiled.find_invalid(rng, *pvk);
    if (bad != std::vector<size_t>{3, 10}) rc = 9;
    // the verdicts are verify_proof's, proof by proof
    for (size_t i : {size_t(0), size_t(3)}) {
      int single = BH_OK;
      try {
        groth16::verify_proof(*pvk, proofs[i], {i == 3 ? circuits[i].image() + Fr::from_u64(1) : circuits[i].image()});
      } catch (const groth16::VerificationError &e) {
        single = e.code;
      }
      if (single != v[i]) rc = 10;
    }
    // a wrong input count is refused before any work
    groth16::BatchVerifier wrong;
    wrong.queue(proofs[0], {});
    try {
      wrong.verify_each(*pvk);
      rc = 11;
    } catch (const groth16::VerificationError &e) {
      if (e.code != BH_ERR_INVALID_VERIFYING_KEY) rc = 12;
    }
  } catch (const groth16::VerificationError &e) {
    fprintf(stderr, "VerificationError %d\n", e.code);
    rc = 21;
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 20;
  }
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("verify_each ok\n");
  return rc;
}
