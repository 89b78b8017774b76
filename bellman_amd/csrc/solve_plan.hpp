// Host-only plan of the witness solver (r1cs_solve.hip): which constraint or hint DEFINES each variable that the caller does
// not supply, and the dependency level of every definition.  No device code and no library state: the test library runs the
// planner on caller arrays without a GPU (bh_test_r1cs_solve_plan, tests/test_r1cs_solve_model_cpu.py restates the rule in
// Python integers).  The field arithmetic the rule needs - is a coefficient zero, the sum of a variable's coefficients, is it
// +-1, its inverse - comes in through the template argument F, so the header names no field:
//   F::Elem;  bool is_zero(e);  Elem add(a, b);  bool is_one(e);  bool is_minus_one(e);  Elem inv(e)  (e != 0);  Elem zero()
//
// The rule (variable indices are those of bh_csr.var: 0 is ONE, inputs first, aux behind them; a term whose coefficient-table
// entry is zero does not exist for the plan, as for prover.rs:31 and the densities):
//   known from the start   ONE, every supplied variable, every output variable of a hint
//   one sweep, in order    constraint i defines v when v is the only variable of A_i, B_i, C_i not yet known, v has no term in
//                          A_i or B_i, and the sum s_v of v's coefficients in C_i is not zero; v is known from constraint
//                          i + 1 on.  Every other constraint defines nothing (all known: a check).  No second sweep.
//   value                  v = (<A_i, w> <B_i, w> - sum over the terms of C_i with another variable) / s_v
//   levels                 0 for ONE and supplied variables; a definition is 1 + the highest level among the variables it reads
//                          (a constraint: its other variables; a hint: the variables of its combination); its outputs have
//                          the definition's level.  A hint may read what a later constraint defines; a cycle is refused.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace bh {

constexpr uint32_t SOLVE_HINT_BITS = 1, SOLVE_HINT_INV_OR_ZERO = 2;   // BH_HINT_* of include/bellman_hip.h
constexpr int SOLVE_OK = 0, SOLVE_INVALID = -2;                        // BH_OK, BH_ERR_INVALID_ARG
constexpr uint32_t SOLVE_NO_VAR = 0xFFFFFFFFu;

struct SolveHint {   // the layout of bh_witness_hint
  uint32_t kind, lc_begin, lc_end, out_begin, out_end, shift;
};
struct SolveCsr {    // the layout of bh_csr
  const uint32_t *row_ptr, *var, *coeff;
};

enum : uint32_t { SOLVE_DEF_CONSTRAINT = 0, SOLVE_DEF_BITS = 1, SOLVE_DEF_INV_OR_ZERO = 2 };
enum : uint32_t { SOLVE_S_ONE = 0, SOLVE_S_MINUS_ONE = 1, SOLVE_S_GENERAL = 2 };
// One definition, 32 bytes: the kernels read it as two 16-byte words.
//   constraint   index = the constraint, var = the variable it defines, mode = SOLVE_S_*, a = entry of sinv (SOLVE_S_GENERAL)
//   hint         index = the hint, var = out_begin, count = outputs, mode = shift, a = lc_begin, b = lc_end
struct SolveDef {
  uint32_t kind, index, var, mode, a, b, count, level;
};

// who defines a variable: nobody (ONE, supplied), constraint `index`, or hint `index`
enum : uint32_t { SOLVE_BY_NONE = 0, SOLVE_BY_CONSTRAINT = 1, SOLVE_BY_HINT = 2 };

template <class Elem>
struct SolvePlan {
  int status = SOLVE_OK;
  uint32_t first_unsolved = SOLVE_NO_VAR;   // with SOLVE_INVALID: the variable the refusal names, or SOLVE_NO_VAR
  std::vector<uint8_t> by;                  // per variable: SOLVE_BY_*
  std::vector<uint32_t> by_index;           // per variable: the constraint or the hint
  std::vector<uint32_t> level;              // per variable
  std::vector<SolveDef> defs;               // sorted by level
  std::vector<uint32_t> level_ptr;          // definitions of level l + 1 are defs[level_ptr[l] .. level_ptr[l + 1])
  std::vector<Elem> sinv;                   // 1 / s_v of the SOLVE_S_GENERAL definitions
  size_t n_supplied = 0, n_defined = 0, n_hinted = 0, widest = 0;
};

struct SolveDesc {   // the arrays of bh_solver_desc
  const uint32_t *supplied;
  size_t n_supplied;
  const SolveHint *hints;
  size_t n_hints;
  const uint32_t *lc_var, *lc_coeff;
  size_t n_lc;        // terms in the pool = the largest lc_end
  const uint32_t *out_var;
  size_t n_out;       // entries of out_var = the largest out_end
};

// coeffs / hint_coeffs: the circuit's and the hints' coefficient tables (read for "is it zero" and for the sums s_v)
template <class F>
SolvePlan<typename F::Elem> solve_plan(const F &f, size_t n_vars, size_t n_constraints, const SolveCsr abc[3],
                                       const typename F::Elem *coeffs, size_t n_coeffs, const SolveDesc &d,
                                       const typename F::Elem *hint_coeffs, size_t n_hint_coeffs) {
  typedef typename F::Elem Elem;
  SolvePlan<Elem> p;
  auto refuse = [&](uint32_t var) -> SolvePlan<Elem> & {
    p.status = SOLVE_INVALID;
    p.first_unsolved = var;
    return p;
  };
  if (n_vars == 0 || n_vars >= ((size_t)1 << 32) || n_constraints >= ((size_t)1 << 32)) return refuse(SOLVE_NO_VAR);
  p.by.assign(n_vars, SOLVE_BY_NONE);
  p.by_index.assign(n_vars, 0);
  p.level.assign(n_vars, 0);
  std::vector<uint8_t> known(n_vars, 0), supplied(n_vars, 0);
  std::vector<uint8_t> cz(n_coeffs), hz(n_hint_coeffs);
  for (size_t c = 0; c < n_coeffs; c++) cz[c] = f.is_zero(coeffs[c]);
  for (size_t c = 0; c < n_hint_coeffs; c++) hz[c] = f.is_zero(hint_coeffs[c]);

  known[0] = supplied[0] = 1;   // ONE
  for (size_t i = 0; i < d.n_supplied; i++) {
    if (d.supplied[i] >= n_vars) return refuse(d.supplied[i]);
    if (!supplied[d.supplied[i]]) p.n_supplied++;
    known[d.supplied[i]] = supplied[d.supplied[i]] = 1;
  }
  for (size_t h = 0; h < d.n_hints; h++) {
    const SolveHint &hh = d.hints[h];
    if (hh.lc_begin > hh.lc_end || hh.lc_end > d.n_lc || hh.out_begin >= hh.out_end || hh.out_end > d.n_out) return refuse(SOLVE_NO_VAR);
    const uint32_t count = hh.out_end - hh.out_begin;
    if (hh.kind == SOLVE_HINT_BITS) {
      if (hh.shift > 256 || count > 256 - hh.shift) return refuse(SOLVE_NO_VAR);
    } else if (hh.kind == SOLVE_HINT_INV_OR_ZERO) {
      if (count != 1 || hh.shift != 0) return refuse(SOLVE_NO_VAR);
    } else {
      return refuse(SOLVE_NO_VAR);
    }
    for (uint32_t t = hh.lc_begin; t < hh.lc_end; t++)
      if (d.lc_var[t] >= n_vars || d.lc_coeff[t] >= n_hint_coeffs) return refuse(SOLVE_NO_VAR);
    for (uint32_t o = hh.out_begin; o < hh.out_end; o++) {
      const uint32_t v = d.out_var[o];
      if (v >= n_vars) return refuse(SOLVE_NO_VAR);
      if (supplied[v] || p.by[v] != SOLVE_BY_NONE) return refuse(v);   // ONE, a supplied variable, another hint's output
      p.by[v] = SOLVE_BY_HINT;
      p.by_index[v] = (uint32_t)h;
      known[v] = 1;
      p.n_hinted++;
    }
  }

  // the sweep
  std::vector<uint32_t> def_constraint;   // constraints that define, in order
  std::vector<Elem> def_s;
  for (size_t i = 0; i < n_constraints; i++) {
    uint32_t u = SOLVE_NO_VAR;
    bool many = false, in_ab = false;
    for (int m = 0; m < 3 && !many; m++)
      for (uint32_t t = abc[m].row_ptr[i]; t < abc[m].row_ptr[i + 1]; t++) {
        if (cz[abc[m].coeff[t]]) continue;
        const uint32_t v = abc[m].var[t];
        if (known[v]) continue;
        if (u == SOLVE_NO_VAR) u = v;
        else if (u != v) { many = true; break; }
        if (m < 2) in_ab = true;
      }
    if (u == SOLVE_NO_VAR || many || in_ab) continue;
    Elem s = f.zero();
    for (uint32_t t = abc[2].row_ptr[i]; t < abc[2].row_ptr[i + 1]; t++)
      if (abc[2].var[t] == u && !cz[abc[2].coeff[t]]) s = f.add(s, coeffs[abc[2].coeff[t]]);
    if (f.is_zero(s)) continue;
    known[u] = 1;
    p.by[u] = SOLVE_BY_CONSTRAINT;
    p.by_index[u] = (uint32_t)i;
    def_constraint.push_back((uint32_t)i);
    def_s.push_back(s);
    p.n_defined++;
  }
  for (size_t v = 0; v < n_vars; v++)
    if (!known[v]) return refuse((uint32_t)v);

  // definitions: the defining constraints in order, then the hints
  const size_t n_defs = def_constraint.size() + d.n_hints;
  std::vector<SolveDef> defs(n_defs);
  for (size_t j = 0; j < def_constraint.size(); j++) {
    SolveDef &e = defs[j];
    e = SolveDef();
    e.kind = SOLVE_DEF_CONSTRAINT;
    e.index = def_constraint[j];
    e.count = 1;
    // (the variable: the one whose definer is this constraint - found again below while the inputs are walked)
    if (f.is_one(def_s[j])) e.mode = SOLVE_S_ONE;
    else if (f.is_minus_one(def_s[j])) e.mode = SOLVE_S_MINUS_ONE;
    else {
      e.mode = SOLVE_S_GENERAL;
      e.a = (uint32_t)p.sinv.size();
      p.sinv.push_back(f.inv(def_s[j]));
    }
  }
  for (size_t h = 0; h < d.n_hints; h++) {
    SolveDef &e = defs[def_constraint.size() + h];
    const SolveHint &hh = d.hints[h];
    e = SolveDef();
    e.kind = hh.kind == SOLVE_HINT_BITS ? SOLVE_DEF_BITS : SOLVE_DEF_INV_OR_ZERO;
    e.index = (uint32_t)h;
    e.var = hh.out_begin;
    e.mode = hh.shift;
    e.a = hh.lc_begin;
    e.b = hh.lc_end;
    e.count = hh.out_end - hh.out_begin;
  }
  // the definition of a variable (SOLVE_NO_VAR: level 0)
  std::vector<uint32_t> def_of(n_vars, SOLVE_NO_VAR);
  for (size_t j = 0; j < def_constraint.size(); j++) {
    const uint32_t i = def_constraint[j];
    for (uint32_t t = abc[2].row_ptr[i]; t < abc[2].row_ptr[i + 1]; t++) {
      const uint32_t v = abc[2].var[t];
      if (p.by[v] == SOLVE_BY_CONSTRAINT && p.by_index[v] == i && !cz[abc[2].coeff[t]]) { defs[j].var = v; def_of[v] = (uint32_t)j; }
    }
  }
  for (size_t h = 0; h < d.n_hints; h++)
    for (uint32_t o = d.hints[h].out_begin; o < d.hints[h].out_end; o++) def_of[d.out_var[o]] = (uint32_t)(def_constraint.size() + h);

  // levels in dependency order (Kahn): a definition waits for the definitions of the variables it reads
  auto for_inputs = [&](size_t j, auto &&fn) {
    const SolveDef &e = defs[j];
    if (e.kind == SOLVE_DEF_CONSTRAINT) {
      for (int m = 0; m < 3; m++)
        for (uint32_t t = abc[m].row_ptr[e.index]; t < abc[m].row_ptr[e.index + 1]; t++)
          if (!cz[abc[m].coeff[t]] && abc[m].var[t] != e.var) fn(abc[m].var[t]);
    } else {
      for (uint32_t t = e.a; t < e.b; t++)
        if (!hz[d.lc_coeff[t]]) fn(d.lc_var[t]);
    }
  };
  std::vector<uint32_t> waits(n_defs, 0), user_ptr(n_defs + 1, 0);
  for (size_t j = 0; j < n_defs; j++)
    for_inputs(j, [&](uint32_t v) {
      if (def_of[v] != SOLVE_NO_VAR) { waits[j]++; user_ptr[def_of[v] + 1]++; }
    });
  for (size_t j = 0; j < n_defs; j++) user_ptr[j + 1] += user_ptr[j];
  std::vector<uint32_t> users(user_ptr[n_defs]), cursor(user_ptr.begin(), user_ptr.end() - 1);
  for (size_t j = 0; j < n_defs; j++)
    for_inputs(j, [&](uint32_t v) {
      if (def_of[v] != SOLVE_NO_VAR) users[cursor[def_of[v]]++] = (uint32_t)j;
    });
  std::vector<uint32_t> ready, def_level(n_defs, 0);
  for (size_t j = 0; j < n_defs; j++)
    if (!waits[j]) ready.push_back((uint32_t)j);
  size_t done = 0;
  uint32_t levels = 0;
  while (done < ready.size()) {
    const uint32_t j = ready[done++];
    uint32_t lv = 0;
    for_inputs(j, [&](uint32_t v) {
      if (def_of[v] != SOLVE_NO_VAR && def_level[def_of[v]] > lv) lv = def_level[def_of[v]];
    });
    def_level[j] = lv + 1;
    if (lv + 1 > levels) levels = lv + 1;
    for (uint32_t q = user_ptr[j]; q < user_ptr[j + 1]; q++)
      if (--waits[users[q]] == 0) ready.push_back(users[q]);
  }
  if (done != n_defs) {   // a cycle: the lowest variable whose definition never became ready
    for (size_t v = 0; v < n_vars; v++)
      if (def_of[v] != SOLVE_NO_VAR && def_level[def_of[v]] == 0) return refuse((uint32_t)v);
    return refuse(SOLVE_NO_VAR);
  }
  for (size_t v = 0; v < n_vars; v++)
    if (def_of[v] != SOLVE_NO_VAR) p.level[v] = def_level[def_of[v]];

  // sorted by level (a counting sort: the order inside a level is the order above)
  p.level_ptr.assign((size_t)levels + 1, 0);
  for (size_t j = 0; j < n_defs; j++) p.level_ptr[def_level[j]]++;
  for (uint32_t l = 0; l < levels; l++) {
    if (p.level_ptr[l + 1] > p.widest) p.widest = p.level_ptr[l + 1];
    p.level_ptr[l + 1] += p.level_ptr[l];
  }
  p.defs.resize(n_defs);
  std::vector<uint32_t> at(p.level_ptr.begin(), p.level_ptr.end());
  for (size_t j = 0; j < n_defs; j++) {
    defs[j].level = def_level[j];
    p.defs[at[def_level[j] - 1]++] = defs[j];
  }
  return p;
}

}  // namespace bh
