// A C++ user of the witness solver in the bellman mirror (bellman_amd/csrc/groth16.hpp): five witnesses of the cubic circuit
// of prove_cubic.cpp completed by R1cs::solver / Solver::solve from x alone, compared with the circuit's own synthesis, and
// judged by R1cs::which_is_unsatisfied; a solver with nothing supplied is refused by the name of the first unknown variable.
// Prints "solver ok" and exits 0 when every expectation holds.
#include <stdio.h>
#include <string.h>

#include <stdexcept>
#include <string>
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

int main() {
  bh_ctx *ctx = nullptr;
  if (bh_ctx_create(0, &ctx) != BH_OK) { fprintf(stderr, "no gfx950 device (no CPU fallback)\n"); return 4; }
  int rc = 0;
  try {
    CubicDemo shape;
    shape.x = Fr::zero();
    groth16::R1cs r1cs(shape, ctx);
    const size_t k = 5, ni = r1cs.num_inputs, na = r1cs.num_aux;
    const uint32_t supplied[1] = {(uint32_t)ni};   // x: the first aux variable
    bh_solver_desc desc;
    memset(&desc, 0, sizeof desc);
    desc.supplied = supplied;
    desc.n_supplied = 1;
    std::unique_ptr<groth16::Solver> solver = r1cs.solver(desc);
    if (solver->supplied != 1 || solver->defined != 3 || solver->hinted != 0 || solver->levels != 3 || solver->widest_level != 1) rc = 10;
    std::vector<Fr> inputs(k * ni, Fr::from_u64(77)), aux(k * na, Fr::from_u64(99)), want_in, want_aux;
    for (size_t j = 0; j < k; j++) {
      CubicDemo c;
      c.x = Fr::from_u64(1000 + 17 * j) * Fr::from_u64(0x9E3779B97F4A7C15ULL);
      groth16::WitnessAssignment w;
      w.alloc_input([] { return Fr::one(); });
      c.synthesize(w);
      want_in.insert(want_in.end(), w.input_assignment.begin(), w.input_assignment.end());
      want_aux.insert(want_aux.end(), w.aux_assignment.begin(), w.aux_assignment.end());
      inputs[j * ni] = Fr::one();
      aux[j * na] = c.x;
    }
    solver->solve(inputs.data(), aux.data(), k);
    if (memcmp(inputs.data(), want_in.data(), k * ni * sizeof(Fr)) != 0 || memcmp(aux.data(), want_aux.data(), k * na * sizeof(Fr)) != 0) rc = 11;
    std::vector<groth16::WitnessView> views;
    for (size_t j = 0; j < k; j++) views.push_back(groth16::WitnessView{inputs.data() + j * ni, ni, aux.data() + j * na, na});
    for (uint32_t b : r1cs.which_is_unsatisfied(views.data(), k))
      if (b != BH_R1CS_SATISFIED) rc = 12;
    desc.n_supplied = 0;
    try {
      r1cs.solver(desc);
      rc = 13;
    } catch (const std::invalid_argument &e) {
      if (std::string(e.what()).find("variable 1 ") == std::string::npos) rc = 14;   // the public output, the lowest unknown
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "exception: %s\n", e.what());
    rc = 20;
  }
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("solver ok\n");
  return rc;
}
