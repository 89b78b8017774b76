// A C++ user of the verifier in the bellman mirror (bellman_amd/csrc/groth16.hpp): generate_parameters for the cubic
// circuit of prove_cubic.cpp, proofs by create_random_proof, then prepare_verifying_key / verify_proof /
// batch::Verifier as bellman's groth16 crate offers them.  The generators g1 (96 B) | g2 (192 B) come from a file written
// by tests/test_gpu_verifier_cpp.py.  Prints "verify ok" and exits 0 when every expectation holds.
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

// the VerificationError code a call throws, 0 when it returns
template <class F> static int code_of(F &&f) {
  try {
    f();
    return 0;
  } catch (const groth16::VerificationError &e) {
    return e.code;
  }
}

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
    if (pvk->num_inputs() != 1) rc = 5;
    std::vector<CubicDemo> circuits(6);
    std::vector<groth16::Proof> proofs;
    for (size_t i = 0; i < circuits.size(); i++) {
      circuits[i].x = rand_fr();
      proofs.push_back(groth16::create_random_proof(circuits[i], params, rng));
    }
    // verify_proof: the right image, a wrong one, a wrong number of inputs
    for (size_t i = 0; i < proofs.size(); i++)
      if (code_of([&] { groth16::verify_proof(*pvk, proofs[i], {circuits[i].image()}); }) != 0) rc = 6;
    if (code_of([&] { groth16::verify_proof(*pvk, proofs[0], {circuits[0].image() + Fr::one()}); }) != BH_ERR_INVALID_PROOF) rc = 7;
    if (code_of([&] { groth16::verify_proof(*pvk, proofs[0], {}); }) != BH_ERR_INVALID_VERIFYING_KEY) rc = 8;
    // batch::Verifier: all valid; one wrong image; an item with the wrong input count; empty
    groth16::BatchVerifier good, bad, wrong_count, empty;
    for (size_t i = 0; i < proofs.size(); i++) {
      good.queue(proofs[i], {circuits[i].image()});
      bad.queue(proofs[i], {i == 3 ? circuits[i].image() + Fr::one() : circuits[i].image()});
      wrong_count.queue(proofs[i], i == 5 ? std::vector<Fr>{} : std::vector<Fr>{circuits[i].image()});
    }
    if (code_of([&] { good.verify(rng, *pvk); }) != 0) rc = 9;
    if (code_of([&] { bad.verify(rng, *pvk); }) != BH_ERR_INVALID_PROOF) rc = 10;
    if (code_of([&] { wrong_count.verify(rng, *pvk); }) != BH_ERR_INVALID_VERIFYING_KEY) rc = 11;
    if (code_of([&] { empty.verify(rng, *pvk); }) != 0) rc = 12;
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 20;
  }
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("verify ok\n");
  return rc;
}
