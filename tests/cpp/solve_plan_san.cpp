// The witness solver's planner (bellman_amd/csrc/solve_plan.hpp) on its own, over a toy prime field, for a host sanitizer
// run: tests/test_r1cs_solve_model_cpu.py builds this file with -fsanitize=address,undefined and runs it.  A multiplicative
// chain with every kind of net coefficient, a bit hint and an inverse hint that read late variables, and the refusals
// (unsolved variable, hint onto ONE, hint cycle, malformed hint, supplied index out of range).  Prints "solve_plan ok".
#include <stdio.h>

#include <vector>

#include "../../bellman_amd/csrc/solve_plan.hpp"

struct Toy {   // integers mod 65537
  typedef uint32_t Elem;
  static constexpr uint32_t P = 65537;
  static Elem zero() { return 0; }
  static bool is_zero(Elem a) { return a % P == 0; }
  static Elem add(Elem a, Elem b) { return (a + b) % P; }
  static bool is_one(Elem a) { return a % P == 1; }
  static bool is_minus_one(Elem a) { return a % P == P - 1; }
  static Elem inv(Elem a) {
    uint64_t r = 1, b = a % P;
    for (uint32_t e = P - 2; e; e >>= 1, b = b * b % P)
      if (e & 1) r = r * b % P;
    return (Elem)r;
  }
};

struct Rows {
  std::vector<uint32_t> row_ptr{0}, var, coeff;
  void row(std::initializer_list<std::pair<uint32_t, uint32_t>> terms) {
    for (auto &t : terms) { var.push_back(t.first); coeff.push_back(t.second); }
    row_ptr.push_back((uint32_t)var.size());
  }
  bh::SolveCsr csr() const { return bh::SolveCsr{row_ptr.data(), var.data(), coeff.data()}; }
};

int main() {
  using namespace bh;
  const std::vector<uint32_t> table = {1, 0, Toy::P - 1, 7, 65530};   // coefficient entries: 1, 0, -1, 7, -7
  const size_t n = 60;                                                // variables: ONE, x = 1, then x_2 .. x_57, two hint outputs 58, 59
  Rows a, b, c;
  for (uint32_t v = 2; v < 58; v++) {   // x_{v-1} * x_{v-1} = s * x_v (+ a zero-coefficient mention of a later variable)
    a.row({{v - 1, 0}, {v + 1 < 58 ? v + 1 : v, 1}});
    b.row({{v - 1, 0}});
    if (v % 3 == 0) c.row({{v, 3}, {v, 3}});   // 7 + 7: a general net coefficient over two terms
    else if (v % 3 == 1) c.row({{v, 2}});
    else c.row({{v, 0}});
  }
  const SolveCsr abc[3] = {a.csr(), b.csr(), c.csr()};
  const uint32_t supplied[1] = {1};
  const uint32_t lc_var[3] = {57, 1, 30}, lc_coeff[3] = {0, 3, 1}, out_var[2] = {58, 59};
  SolveHint hints[2] = {{SOLVE_HINT_BITS, 0, 2, 0, 1, 5}, {SOLVE_HINT_INV_OR_ZERO, 2, 3, 1, 2, 0}};
  SolveDesc d{supplied, 1, hints, 2, lc_var, lc_coeff, 3, out_var, 2};
  int rc = 0;
  {
    const SolvePlan<uint32_t> p = solve_plan(Toy(), n, 56, abc, table.data(), table.size(), d, table.data(), table.size());
    if (p.status != SOLVE_OK || p.n_supplied != 1 || p.n_defined != 56 || p.n_hinted != 2) rc = 1;
    else if (p.level[57] != 56 || p.level[58] != 57 || p.level[59] != 1 /* its one term has a zero coefficient: it reads nothing */ || p.level_ptr.size() != 58 || p.widest != 2) rc = 2;
    else if (p.sinv.size() != 19 || (uint64_t)p.sinv[0] * 14 % Toy::P != 1 || p.defs.size() != 58 || p.defs[0].var != 2) rc = 3;
  }
  auto refused = [&](const SolveDesc &dd, uint32_t want) {
    const SolvePlan<uint32_t> p = solve_plan(Toy(), n, 56, abc, table.data(), table.size(), dd, table.data(), table.size());
    return p.status == SOLVE_INVALID && p.first_unsolved == want;
  };
  SolveDesc none = d;
  none.n_supplied = 0;
  if (!refused(none, 1)) rc = 4;                       // x itself
  SolveHint onto_one[1] = {{SOLVE_HINT_BITS, 0, 2, 0, 1, 0}};
  const uint32_t out_one[1] = {0};
  SolveDesc d1{supplied, 1, onto_one, 1, lc_var, lc_coeff, 3, out_one, 1};
  if (!refused(d1, 0)) rc = 5;
  SolveHint cyc[1] = {{SOLVE_HINT_INV_OR_ZERO, 0, 1, 0, 1, 0}};   // x_20 = 1 / x_57, and x_57 descends from x_20
  const uint32_t out_cyc[1] = {20};
  const uint32_t supplied3[3] = {1, 58, 59};
  SolveDesc d2{supplied3, 3, cyc, 1, lc_var, lc_coeff, 3, out_cyc, 1};
  if (!refused(d2, 20)) rc = 6;
  SolveHint wide[1] = {{SOLVE_HINT_BITS, 0, 2, 0, 2, 255}};
  SolveDesc d3{supplied, 1, wide, 1, lc_var, lc_coeff, 3, out_var, 2};
  if (!refused(d3, SOLVE_NO_VAR)) rc = 7;
  const uint32_t far[1] = {60};
  SolveDesc d4{far, 1, nullptr, 0, nullptr, nullptr, 0, nullptr, 0};
  if (!refused(d4, 60)) rc = 8;
  if (rc == 0) printf("solve_plan ok\n");
  return rc;
}
