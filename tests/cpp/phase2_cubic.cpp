// A C++ user of Parameters::verify_step in the bellman mirror (bellman_amd/csrc/groth16.hpp): parameters for the cubic
// circuit of prove_cubic.cpp are derived from a powers-of-tau transcript made on the device, one contributor rescales
// delta, and the receiver's check must pass for that step (and for two steps composed, and for d = 1) and fail with the
// expected bit for three tampered sets: a record of `a` replaced, l taken from another rescaling, delta_g1 from another
// rescaling.  The generators g1 (96 B) | g2 (192 B) come from a file written by tests/test_gpu_phase2_cpp.py.  Prints
// "phase2 ok" and exits 0 when every expectation holds.
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
};

// [scale tau^i] base, i < n, as an owned handle
static bh_bases *powers(bh_ctx *ctx, int group, const void *base, size_t n, const Fr &tau, const Fr &scale) {
  void *sc = nullptr, *pts = nullptr;
  bh_bases *out = nullptr;
  const size_t rec = group == BH_G1 ? 96 : 192;
  if (bh_dev_alloc(ctx, n * 32 + 32, &sc) != BH_OK || bh_dev_alloc(ctx, n * rec + rec, &pts) != BH_OK) exit(30);
  if (bh_fr_powers_dev(ctx, sc, n, &tau, &scale, nullptr) != BH_OK) exit(31);
  if (bh_fixed_base_mul_dev(ctx, group, base, sc, n, BH_SCALARS_MONT, pts, nullptr) != BH_OK) exit(32);
  if (bh_bases_copy_dev(ctx, group, pts, n, &out) != BH_OK) exit(33);
  bh_dev_free(ctx, sc);
  bh_dev_free(ctx, pts);
  return out;
}

// the records of a parameter set on the host, and a set rebuilt from them
struct HostSet {
  groth16::VerifyingKey vk;
  std::vector<groth16::G1Affine> h, l, a, b_g1;
  std::vector<groth16::G2Affine> b_g2;
  explicit HostSet(const groth16::Parameters &p) : vk(p.vk) {
    h.resize(bh_bases_len(p.h)); l.resize(bh_bases_len(p.l)); a.resize(bh_bases_len(p.a)); b_g1.resize(bh_bases_len(p.b_g1));
    b_g2.resize(bh_bases_len(p.b_g2));
    if (bh_bases_download(p.ctx, p.h, 0, h.size(), h.data()) != BH_OK || bh_bases_download(p.ctx, p.l, 0, l.size(), l.data()) != BH_OK ||
        bh_bases_download(p.ctx, p.a, 0, a.size(), a.data()) != BH_OK || bh_bases_download(p.ctx, p.b_g1, 0, b_g1.size(), b_g1.data()) != BH_OK ||
        bh_bases_download(p.ctx, p.b_g2, 0, b_g2.size(), b_g2.data()) != BH_OK)
      exit(34);
  }
  std::unique_ptr<groth16::Parameters> upload(bh_ctx *ctx) const {
    return std::unique_ptr<groth16::Parameters>(new groth16::Parameters(ctx, vk, h.data(), h.size(), l.data(), l.size(), a.data(), a.size(),
                                                                        b_g1.data(), b_g1.size(), b_g2.data(), b_g2.size()));
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
  uint64_t state = 0x9E3779B97F4A7C15ULL;
  auto rng = [&state] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto rand_fr = [&] { uint64_t w[8]; for (uint64_t &x : w) x = rng(); return Fr::from_u512(w); };
  unsigned char seed[32];
  for (unsigned char &b : seed) b = (unsigned char)rng();   // (a test: a verifier draws it from a CSPRNG, after the upload)
  std::vector<bh_bases *> handles;
  try {
    CubicDemo shape;
    shape.x = Fr::zero();
    groth16::R1cs r1cs(shape, ctx);
    const Fr alpha = rand_fr(), beta = rand_fr(), tau = rand_fr(), d = rand_fr(), d2 = rand_fr(), one = Fr::one();
    size_t m = 1;
    while (m < r1cs.num_constraints) m *= 2;
    groth16::PowersOfTau t;
    handles.push_back(powers(ctx, BH_G1, &g1, 2 * m - 1, tau, one));
    handles.push_back(powers(ctx, BH_G2, &g2, m, tau, one));
    handles.push_back(powers(ctx, BH_G1, &g1, m, tau, alpha));
    handles.push_back(powers(ctx, BH_G1, &g1, m, tau, beta));
    t.tau_g1 = handles[0]; t.tau_g2 = handles[1]; t.alpha_tau_g1 = handles[2]; t.beta_tau_g1 = handles[3];
    uint64_t bc[4];
    beta.to_canonical(bc);
    bh_point_mul(BH_G2, &t.beta_g2, &g2, bc);
    groth16::Parameters first(ctx, r1cs, t);
    std::unique_ptr<groth16::Parameters> second = first.rescale_delta(d), third = second->rescale_delta(d2);
    // honest steps: one, two composed, d = 1, with and without the point validation
    for (unsigned flags : {0u, BH_STEP_VALIDATE_POINTS}) {
      if (!first.verify_step(*second, seed, flags).ok()) rc = 5;
      if (!second->verify_step(*third, seed, flags).ok()) rc = 6;
      if (!first.verify_step(*third, seed, flags).ok()) rc = 7;
      if (!first.verify_step(first, seed, flags).ok()) rc = 8;
    }
    if (!first.verify_step(*second, seed).ok()) rc = 9;   // the default: validate
    // a record of `a` replaced by its neighbour
    {
      HostSet s(*second);
      if (s.a.size() < 2 || !memcmp(&s.a[0], &s.a[1], 96)) rc = 10;
      s.a[0] = s.a[1];
      const groth16::Parameters::StepCheck c = first.verify_step(*s.upload(ctx), seed);
      if (c.code != BH_ERR_INVALID_TRANSCRIPT || c.report.failed != BH_STEP_FAILED_A || c.report.bad_vector != 1 || c.report.bad_index != 0) rc = 11;
    }
    // l from the rescaling by d d2, everything else from the one by d
    {
      HostSet s(*second);
      s.l = HostSet(*third).l;
      const groth16::Parameters::StepCheck c = first.verify_step(*s.upload(ctx), seed);
      if (c.code != BH_ERR_INVALID_TRANSCRIPT || c.report.failed != BH_STEP_FAILED_L) rc = 12;
    }
    // delta_g1 from the other rescaling: H and L relate to delta_g2 and still hold
    {
      HostSet s(*second);
      s.vk.delta_g1 = third->vk.delta_g1;
      const groth16::Parameters::StepCheck c = first.verify_step(*s.upload(ctx), seed, 0);
      if (c.code != BH_ERR_INVALID_TRANSCRIPT || c.report.failed != BH_STEP_FAILED_DELTA) rc = 13;
    }
    // an untouched round trip through the host passes: equal points are equal records
    if (!first.verify_step(*HostSet(*second).upload(ctx), seed).ok()) rc = 14;
    try {
      first.verify_step(*second, seed, 2u);
      rc = 15;
    } catch (const std::invalid_argument &) {
    }
  } catch (const SynthesisError &e) {
    fprintf(stderr, "SynthesisError %d: %s\n", e.code, e.what());
    rc = 20;
  } catch (const std::exception &e) {
    fprintf(stderr, "exception: %s\n", e.what());
    rc = 21;
  }
  for (bh_bases *b : handles) bh_bases_release(ctx, b);
  bh_ctx_destroy(ctx);
  if (rc == 0) printf("phase2 ok\n");
  return rc;
}
