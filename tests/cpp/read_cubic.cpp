// A C++ user of Proof::read in the bellman mirror (bellman_amd/csrc/groth16.hpp): proofs of the cubic circuit of
// prove_cubic.cpp by create_random_proof, written with Proof::write, read back with Proof::read (decompression and
// subgroup checks on the device) and verified; a damaged proof must raise the reader's IoError.  The generators g1 (96 B)
// | g2 (192 B) come from a file written by tests/test_gpu_proof_read_cpp.py.  Prints "read ok" and exits 0 when every
// expectation holds.
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
    std::vector<CubicDemo> circuits(4);
    std::vector<groth16::Proof> proofs;
    std::vector<unsigned char> bytes(192 * circuits.size());
    for (size_t i = 0; i < circuits.size(); i++) {
      circuits[i].x = rand_fr();
      proofs.push_back(groth16::create_random_proof(circuits[i], params, rng));
      proofs[i].write(&bytes[192 * i]);
    }
    // one proof, then all of them: identical records, and they verify
    const groth16::Proof one = groth16::Proof::read(ctx, &bytes[0]);
    if (memcmp(&one, &proofs[0], sizeof one) != 0) rc = 5;
    const std::vector<groth16::Proof> all = groth16::Proof::read(ctx, bytes.data(), circuits.size());
    for (size_t i = 0; i < all.size(); i++) {
      if (memcmp(&all[i], &proofs[i], sizeof(groth16::Proof)) != 0) rc = 6;
      groth16::verify_proof(*pvk, all[i], {circuits[i].image()});
    }
    // a cleared compression flag on B of proof 2; an identity A in proof 1 (the earlier proof is the one reported)
    std::vector<unsigned char> damaged = bytes;
    damaged[192 * 2 + 48] &= 0x7f;
    size_t bad = 99;
    try {
      groth16::Proof::read(ctx, damaged.data(), circuits.size(), &bad);
      rc = 7;
    } catch (const IoError &e) {
      if (e.code != BH_ERR_INVALID_POINT || bad != 2 || strcmp(e.what(), "invalid G2") != 0) rc = 8;
    }
    memset(&damaged[192], 0, 48);
    damaged[192] = 0xC0;
    try {
      groth16::Proof::read(ctx, damaged.data(), circuits.size(), &bad);
      rc = 9;
    } catch (const IoError &e) {
      if (e.code != BH_ERR_POINT_AT_INFINITY || bad != 1) rc = 10;
    }
  } catch (const groth16::VerificationError &e) {
    fprintf(stderr, "VerificationError %d\n", e.code);
    rc = 21;
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 20;
  }
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("read ok\n");
  return rc;
}
