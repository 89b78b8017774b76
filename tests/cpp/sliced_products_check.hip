// Host check of the products over SLICED operands (bellman_amd/csrc/ff.cuh: fe_to_hform, fe_mul_hh, fe_sqr_h, fe_mul2_hh and
// the FpOps entry points mul_hh / sqr_h / mul2_sub_tail_h, whose out-of-line bodies take the limbs in registers) and of the
// mixed addition built on them (ec.cuh xyzz_madd_sliced).  The claim is equality WORD FOR WORD with what
// the G1 bucket accumulation called before: fe_mul, fe_sqr, fe_mul2, FpOps::mul / sqr / mul2_sub_tail and xyzz_madd - no
// canonicalisation before the comparison, lazily reduced and canonical forms of the reduction both.
// Operands: 0, 1, p - 1, p, the Montgomery one, 2p - 1 (the largest lazily reduced value), a value below 2^381 with every 30-bit
// limb of every sliced form at 2^30 - 1, all 384 bits set (single products only: the reduction takes any words), every pair /
// quadruple of those, and 10 000 random pairs / quadruples below 2p.  For the fused tail c = 0 makes 2p - c = 2p, the largest
// operand it admits.
// The field and curve code is __host__ __device__: nothing here runs on a device.  Built (with ASan + UBSan on the host
// side where the compiler has them) and run by tests/test_sliced_products_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bellman_amd/csrc/ec.cuh"

using namespace bh;

static uint64_t sm_state = 0x243F6A8885A308D3ull;
static uint64_t splitmix() {
  uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fp_t random_below_2p() {
  for (;;) {
    fp_t r;
    for (int i = 0; i < 12; i += 2) { const uint64_t v = splitmix(); r.l[i] = (u32)v; r.l[i + 1] = (u32)(v >> 32); }
    r.l[11] &= 0x3fffffffu;   // < 2^382
    for (int i = 11; i >= 0; i--)
      if (r.l[i] != fp_mod2(i)) { if (r.l[i] < fp_mod2(i)) return r; break; }
  }
}
static bool words_equal(const fp_t &a, const fp_t &b) { return memcmp(&a, &b, sizeof a) == 0; }

static int bad = 0;
static void fail(const char *what, size_t i, size_t j) {
  if (bad++ < 10) printf("%s differs at (%zu, %zu)\n", what, i, j);
}

// every single product / squaring form on one pair
static void check_pair(const fp_t &a, const fp_t &b, size_t i, size_t j) {
  fp_h ha, hb;
  FpOps::slice(ha, a);
  FpOps::slice(hb, b);
  for (int k = 0; k < 13; k++)
    if ((ha.l[k] | hb.l[k]) >> 30) fail("limb above 30 bits", i, j);
  fp_t want, got;
  fe_mul<FpParams, false>(want, a, b);
  fe_mul_hh<FpParams, false>(got, ha.l, hb.l);
  if (!words_equal(want, got)) fail("fe_mul_hh (lazy)", i, j);
  FpOps::mul_hh(got, ha, hb);
  if (!words_equal(want, got)) fail("FpOps::mul_hh", i, j);
  FpOps::mul(want, a, b);
  if (!words_equal(want, got)) fail("FpOps::mul_hh vs FpOps::mul", i, j);
  fe_mul<FpParams, true>(want, a, b);
  fe_mul_hh<FpParams, true>(got, ha.l, hb.l);
  if (!words_equal(want, got)) fail("fe_mul_hh (canonical)", i, j);
  fe_sqr<FpParams, false>(want, a);
  fe_sqr_h<FpParams, false>(got, ha.l);
  if (!words_equal(want, got)) fail("fe_sqr_h (lazy)", i, j);
  FpOps::sqr_h(got, ha);
  if (!words_equal(want, got)) fail("FpOps::sqr_h", i, j);
  fe_sqr<FpParams, true>(want, a);
  fe_sqr_h<FpParams, true>(got, ha.l);
  if (!words_equal(want, got)) fail("fe_sqr_h (canonical)", i, j);
}
// the fused forms on one quadruple; operands below 2^382 (what the fused tail is fed with: values in [0, 2p])
static void check_quad(const fp_t &a, const fp_t &b, const fp_t &c, const fp_t &d, size_t i, size_t j) {
  fp_h ha, hb, hc, hd;
  FpOps::slice(ha, a);
  FpOps::slice(hb, b);
  FpOps::slice(hc, c);
  FpOps::slice(hd, d);
  fp_t want, got;
  fe_mul2<FpParams, false>(want, a, b, c, d);
  fe_mul2_hh<FpParams, false>(got, ha.l, hb.l, hc.l, hd.l);
  if (!words_equal(want, got)) fail("fe_mul2_hh (lazy)", i, j);
  fe_mul2<FpParams, true>(want, a, b, c, d);
  fe_mul2_hh<FpParams, true>(got, ha.l, hb.l, hc.l, hd.l);
  if (!words_equal(want, got)) fail("fe_mul2_hh (canonical)", i, j);
  FpOps::mul2_sub_tail(want, a, b, c, d);
  FpOps::mul2_sub_tail_h(got, ha, b, c, hd);
  if (!words_equal(want, got)) fail("FpOps::mul2_sub_tail_h", i, j);
}

static const u32 GX[12] = {0xfd530c16u, 0x5cb38790u, 0x9976fff5u, 0x7817fc67u, 0x143ba1c1u, 0x154f95c7u,
                           0xf3d0e747u, 0xf0ae6acdu, 0x21dbf440u, 0xedce6eccu, 0x9e0bfb75u, 0x12017741u};
static const u32 GY[12] = {0x0ce72271u, 0xbaac93d5u, 0x7918fd8eu, 0x8c22631au, 0x570725ceu, 0xdd595f13u,
                           0x50405194u, 0x51ac5829u, 0xad0059c0u, 0x0e1c8c3fu, 0x5008a26au, 0x0bbc3efcu};
static Affine<FpOps> to_affine(const XYZZ<FpOps> &p) {
  Affine<FpOps> a;
  if (xyzz_is_identity(p)) { fe_zero(a.x); fe_zero(a.y); return a; }
  fp_t izz, izzz;
  FpOps::inv(izz, p.zz);
  FpOps::inv(izzz, p.zzz);
  FpOps::mul(a.x, p.x, izz);
  FpOps::mul(a.y, p.y, izzz);
  fpl_canon(a.x, a.x);
  fpl_canon(a.y, a.y);
  return a;
}
static bool same_words(const XYZZ<FpOps> &a, const XYZZ<FpOps> &b) { return memcmp(&a, &b, sizeof a) == 0; }

// the mixed addition: the sliced one against xyzz_madd, every coordinate word
static void check_group() {
  Affine<FpOps> gen;
  for (int i = 0; i < 12; i++) { gen.x.l[i] = GX[i]; gen.y.l[i] = GY[i]; }
  constexpr int NP = 40;
  Affine<FpOps> pts[NP];
  {
    XYZZ<FpOps> g1, acc;
    xyzz_from_affine(g1, gen);
    acc = g1;
    for (int i = 0; i < NP; i++) {
      pts[i] = to_affine(acc);
      XYZZ<FpOps> t;
      for (int r = 0; r < 1 + (i % 3); r++) { xyzz_add(t, acc, g1); acc = t; }
      if (i % 7 == 3) { xyzz_dbl(t, acc); acc = t; }
    }
  }
  XYZZ<FpOps> ref, chk;   // xyzz_madd, the sliced addition
  xyzz_set_identity(ref);
  xyzz_set_identity(chk);
  auto step = [&](const Affine<FpOps> &q, size_t at) {
    const bool r_ref = xyzz_madd(ref, q);
    const bool r_chk = xyzz_madd_sliced(chk, q);
    if (r_ref != r_chk || !same_words(ref, chk)) fail("xyzz_madd_sliced", at, 0);
  };
  size_t at = 0;
  for (int round = 0; round < 3; round++) {
    for (int i = 0; i < NP; i++) {
      Affine<FpOps> q = pts[(i * 7 + round) % NP];
      if ((i + round) % 5 == 2) FpOps::neg(q.y, q.y);
      fpl_canon(q.y, q.y);
      step(q, at++);
      if (i % 9 == 4) {   // acc == q: the doubling branch (accumulator with ZZ = ZZZ = 1 right after an opener, general otherwise)
        const Affine<FpOps> same_pt = to_affine(ref);
        step(same_pt, at++);
      }
      if (i % 11 == 6) {  // acc == -q: the identity; the next step is a copy again
        Affine<FpOps> neg_pt = to_affine(ref);
        FpOps::neg(neg_pt.y, neg_pt.y);
        fpl_canon(neg_pt.y, neg_pt.y);
        step(neg_pt, at++);
        if (!xyzz_is_identity(ref) || !xyzz_is_identity(chk)) fail("inverse path", at, 0);
        step(pts[i], at++);
        step(pts[i], at++);   // P then P: doubling of an accumulator with ZZ = ZZZ = 1
      }
    }
  }
}

int main() {
  fp_t zero, one, pm1, p, mont1, twop1, top, allones;
  fe_zero(zero);
  fe_zero(one);
  one.l[0] = 1;
  fe_one(mont1);
  u32 br = 0;
  for (int i = 0; i < 12; i++) {
    p.l[i] = FpParams::mod(i);
    pm1.l[i] = subb(FpParams::mod(i), i == 0 ? 1u : 0u, br, br);
    allones.l[i] = 0xffffffffu;
  }
  br = 0;
  for (int i = 0; i < 12; i++) twop1.l[i] = subb(fp_mod2(i), i == 0 ? 1u : 0u, br, br);
  top = allones;
  top.l[11] = 0x1fffffffu;   // < 2^381: limbs 0..11 of top << 3 are 2^30 - 1 but for the three shifted-in zeros
  std::vector<fp_t> corners = {zero, one, pm1, p, mont1, twop1, top};
  std::vector<fp_t> singles = corners;
  singles.push_back(allones);
  for (size_t i = 0; i < singles.size(); i++)
    for (size_t j = 0; j < singles.size(); j++) check_pair(singles[i], singles[j], i, j);
  for (size_t i = 0; i < corners.size(); i++)
    for (size_t j = 0; j < corners.size(); j++)
      for (size_t k = 0; k < corners.size(); k++)
        for (size_t l = 0; l < corners.size(); l++) check_quad(corners[i], corners[j], corners[k], corners[l], i * 7 + j, k * 7 + l);
  for (size_t it = 0; it < 10000; it++) {
    const fp_t a = random_below_2p(), b = random_below_2p(), c = random_below_2p(), d = random_below_2p();
    check_pair(a, b, 1000 + it, 0);
    check_quad(a, b, c, d, 1000 + it, 1);
    // a corner on one side of a random operand
    check_pair(corners[it % corners.size()], b, 1000 + it, 2);
    check_quad(a, corners[it % corners.size()], corners[(it / 7) % corners.size()], d, 1000 + it, 3);
  }
  check_group();
  printf(bad ? "FAILED %d\n" : "sliced products: ok\n", bad);
  return bad ? 1 : 0;
}
