// A C++ user of the witness check in the bellman mirror (bellman_amd/csrc/groth16.hpp): seven witnesses of the cubic circuit
// of prove_cubic.cpp, each in vectors of its own (so no witness starts where the one before ends), two of them with a wrong
// wire.  R1cs::which_is_unsatisfied names the first unsatisfied constraint of each; prove_witness_batch_checked gives the
// satisfied ones exactly the proofs of prove_witness, the others code 11 and no proof, and throws SynthesisError
// "Unsatisfiable" in its vector form; BATCH_GROUPED_HE (the batched constraint evaluation, here through its per-witness
// upload branch) gives the proofs of prove_witness with the default budget and with one that cuts the batch into groups of
// 2, 2, 2, 1.  The generators g1 (96 B) | g2 (192 B) come from a file written by tests/test_gpu_prove_batch_checked.py.
// Prints "prove_witness_batch_checked ok" and exits 0 when every expectation holds.
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
    const size_t k = 7;
    std::vector<groth16::WitnessAssignment> ws(k);
    std::vector<groth16::WitnessView> views;
    std::vector<std::pair<Fr, Fr>> rs;
    for (size_t j = 0; j < k; j++) {
      CubicDemo c;
      c.x = rand_fr();
      ws[j].alloc_input([] { return Fr::one(); });
      c.synthesize(ws[j]);
      rs.emplace_back(rand_fr(), rand_fr());
    }
    // aux = [x, x^2, x^3]: a wrong x^3 breaks constraint 1 (x^2 * x = x^3) first, a wrong output only constraint 2
    ws[2].aux_assignment[2] = ws[2].aux_assignment[2] + Fr::one();
    ws[5].input_assignment[1] = ws[5].input_assignment[1] + Fr::one();
    std::vector<groth16::Proof> want(k);
    for (size_t j = 0; j < k; j++) {
      views.push_back(groth16::WitnessView{ws[j].input_assignment.data(), ws[j].input_assignment.size(),
                                           ws[j].aux_assignment.data(), ws[j].aux_assignment.size()});
      want[j] = groth16::prove_witness(r1cs, params, views[j].inputs, views[j].n_inputs, views[j].aux, views[j].n_aux, rs[j].first,
                                       rs[j].second);
    }
    const std::vector<uint32_t> expect = {BH_R1CS_SATISFIED, BH_R1CS_SATISFIED, 1, BH_R1CS_SATISFIED, BH_R1CS_SATISFIED, 2, BH_R1CS_SATISFIED};
    if (r1cs.which_is_unsatisfied(views.data(), k) != expect) rc = 5;
    if (!r1cs.which_is_unsatisfied(views.data(), 0).empty()) rc = 5;
    // the codes form: 11 and no proof for the two bad witnesses, prove_witness's proof for the others
    std::vector<Fr> r(k), s(k);
    for (size_t j = 0; j < k; j++) { r[j] = rs[j].first; s[j] = rs[j].second; }
    std::vector<groth16::Proof> got(k);
    std::vector<int> codes(k, -100);
    std::vector<uint32_t> first(k, 12345);
    groth16::prove_witness_batch_checked_codes(r1cs, params, views.data(), k, r.data(), s.data(), got.data(), codes.data(), first.data());
    if (first != expect) rc = 6;
    for (size_t j = 0; j < k && !rc; j++) {
      const bool bad = expect[j] != BH_R1CS_SATISFIED;
      if (codes[j] != (bad ? BH_ERR_UNSATISFIABLE : BH_OK)) rc = 7;
      if (!bad && memcmp(&got[j], &want[j], sizeof want[j]) != 0) rc = 8;
    }
    // the vector form throws for the first bad witness, after reporting every witness
    bool thrown = false;
    std::vector<uint32_t> reported;
    try {
      (void)groth16::prove_witness_batch_checked(r1cs, params, views, rs, &reported);
    } catch (const SynthesisError &e) {
      thrown = e.code == BH_ERR_UNSATISFIABLE && strcmp(e.what(), "Unsatisfiable") == 0;
    }
    if (!thrown || reported != expect) rc = rc ? rc : 9;
    // ... and returns every proof when all witnesses are satisfied
    std::vector<groth16::WitnessView> good_views;
    std::vector<std::pair<Fr, Fr>> good_rs;
    std::vector<size_t> good;
    for (size_t j = 0; j < k; j++)
      if (expect[j] == BH_R1CS_SATISFIED) { good.push_back(j); good_views.push_back(views[j]); good_rs.push_back(rs[j]); }
    const std::vector<groth16::Proof> all = groth16::prove_witness_batch_checked(r1cs, params, good_views, good_rs);
    for (size_t i = 0; i < good.size() && !rc; i++)
      if (memcmp(&all[i], &want[good[i]], sizeof want[0]) != 0) rc = 10;
    // BATCH_GROUPED_HE over witnesses that are not adjacent in host memory: the per-witness upload branch.  The unchecked
    // prover accepts the two bad witnesses as it always did (their proofs are prove_witness's, and do not verify).
    // (m = 8: a budget of 4 * 2 * 8 * 32 bytes holds a, b, c and a scratch vector of two witnesses - groups of 2, 2, 2, 1)
    for (size_t budget : {size_t(0), size_t(4 * 2 * 8 * 32)}) {
      const std::vector<groth16::Proof> he = groth16::prove_witness_batch(r1cs, params, views, rs, nullptr, budget, groth16::BATCH_GROUPED_HE);
      if (he.size() != k) rc = rc ? rc : 11;
      for (size_t j = 0; j < k && !rc; j++)
        if (memcmp(&he[j], &want[j], sizeof want[j]) != 0) { fprintf(stderr, "mode 3 proof %zu differs (budget %zu)\n", j, budget); rc = 12; }
    }
    std::vector<groth16::WitnessView> bad = views;
    bad[2].n_aux -= 1;
    bool refused = false;
    try { (void)r1cs.which_is_unsatisfied(bad.data(), k); } catch (const std::invalid_argument &) { refused = true; }
    if (!refused) rc = rc ? rc : 13;
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 30 + e.code;
  }
  bh_ctx_destroy(ctx);
  if (!rc) printf("prove_witness_batch_checked ok\n");
  return rc;
}
