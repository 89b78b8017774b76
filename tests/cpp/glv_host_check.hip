// Host check of the split-scalar point multiplier (bellman_amd/csrc/glv.cuh) in a program of its own, so that it can run
// under ASan + UBSan without Python: glv_split over the corner scalars and 10 000 random ones against the defining
// identity (k1 + k2 lambda = k as integers, k1 < lambda), and xyzz_mul_glv of both groups against the plain ladder -
// canonical splits against double-and-add over the 255 bits of k, arbitrary pairs (all-one halves, a pair that doubles
// through the mixed addition) against [k1] P + [k2] ([lambda] P).  The field and curve code is __host__ __device__: nothing
// here runs on a device.  Built and run by tests/test_glv_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bellman_amd/csrc/glv.cuh"

using namespace bh;

struct U256 {
  u32 l[8];
};
static U256 from_u64(uint64_t v) {
  U256 r{};
  r.l[0] = (u32)v;
  r.l[1] = (u32)(v >> 32);
  return r;
}
static U256 add(const U256 &a, const U256 &b) {
  U256 r;
  u32 c = 0;
  for (int i = 0; i < 8; i++) r.l[i] = addc(a.l[i], b.l[i], c, c);
  return r;
}
static U256 sub(const U256 &a, const U256 &b) {
  U256 r;
  u32 br = 0;
  for (int i = 0; i < 8; i++) r.l[i] = subb(a.l[i], b.l[i], br, br);
  return r;
}
static U256 mul(const U256 &a, const U256 &b) {   // mod 2^256
  U256 r{};
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
    for (int j = 0; i + j < 8; j++) {
      const uint64_t t = (uint64_t)a.l[i] * b.l[j] + r.l[i + j] + carry;
      r.l[i + j] = (u32)t;
      carry = t >> 32;
    }
  }
  return r;
}
static bool less(const U256 &a, const U256 &b) {
  for (int i = 7; i >= 0; i--)
    if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
  return false;
}
static U256 shl(const U256 &a, int bits) {
  U256 r{};
  for (int i = 0; i < 256 - bits; i++)
    if ((a.l[i >> 5] >> (i & 31)) & 1u) r.l[(i + bits) >> 5] |= 1u << ((i + bits) & 31);
  return r;
}
static U256 widen(const glv_half &h) {
  U256 r{};
  for (int i = 0; i < 4; i++) r.l[i] = h.l[i];
  return r;
}
static glv_half low_half(const U256 &a) {
  glv_half h;
  for (int i = 0; i < 4; i++) h.l[i] = a.l[i];
  return h;
}

static uint64_t sm_state = 0x13198A2E03707344ull;
static uint64_t splitmix() {
  uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int bad = 0;
static void fail(const char *what, size_t i) {
  if (bad++ < 10) printf("%s fails at %zu\n", what, i);
}

// the plain MSB-first ladder over `bits` bits (point_fft.hip's xyzz_mul_fr)
template <class F>
__attribute__((noinline)) static XYZZ<F> ladder(const XYZZ<F> &p, const U256 &k, int bits) {
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  for (int i = bits - 1; i >= 0; i--) {
    xyzz_dbl(acc, acc);
    if ((k.l[i >> 5] >> (i & 31)) & 1u) xyzz_add(acc, acc, p);
  }
  return acc;
}
// (the force-inlined curve code is instantiated once per helper, not once per call: the build under sanitizers stays short)
template <class F>
__attribute__((noinline)) static XYZZ<F> glv_pair(const Affine<F> &p, const glv_half &k1, const glv_half &k2) {
  XYZZ<F> r;
  xyzz_mul_glv(r, p, k1, k2);
  return r;
}
template <class F>
__attribute__((noinline)) static Affine<F> to_affine(const XYZZ<F> &p) {
  Affine<F> a;
  xyzz_to_affine(a, p);
  return a;
}
template <class F>
static bool same_point(const XYZZ<F> &a, const XYZZ<F> &b) {
  const Affine<F> x = to_affine(a), y = to_affine(b);
  return memcmp(&x, &y, sizeof x) == 0;
}
template <class F>
static void check_ladder(const Affine<F> &gen, const std::vector<U256> &scalars, const U256 &lambda) {
  XYZZ<F> g;
  xyzz_from_affine(g, gen);
  // a few points of the subgroup, and the identity
  std::vector<Affine<F>> pts;
  XYZZ<F> acc = g;
  for (int i = 0; i < 5; i++) {
    pts.push_back(to_affine(acc));
    XYZZ<F> t;
    xyzz_dbl(t, acc);
    xyzz_add(acc, t, g);
  }
  for (size_t i = 0; i < scalars.size(); i++) {
    const Affine<F> &p = pts[i % pts.size()];
    XYZZ<F> px;
    xyzz_from_affine(px, p);
    fr_t k;
    memcpy(&k, &scalars[i], sizeof k);
    glv_half k1, k2;
    glv_split(k, k1, k2);
    const XYZZ<F> got = glv_pair(p, k1, k2);
    if (!same_point(got, ladder(px, scalars[i], 255))) fail("xyzz_mul_glv (canonical split)", i);
  }
  // arbitrary pairs against [k1] P + [k2] ([lambda] P)
  const U256 ones = sub(shl(from_u64(1), 128), from_u64(1));
  const U256 lam1 = add(lambda, from_u64(1));
  const U256 pairs[][2] = {{ones, ones}, {ones, from_u64(0)}, {from_u64(0), ones}, {from_u64(3), lam1},   // (3, lambda + 1): 2 s = P, then + P
                           {from_u64(0), from_u64(0)}, {lambda, lambda}};
  for (size_t i = 0; i < sizeof pairs / sizeof pairs[0]; i++) {
    const Affine<F> &p = pts[i % pts.size()];
    XYZZ<F> px, want;
    xyzz_from_affine(px, p);
    const XYZZ<F> got = glv_pair(p, low_half(pairs[i][0]), low_half(pairs[i][1]));
    const XYZZ<F> lp = ladder(px, lambda, 128);
    xyzz_add(want, ladder(px, pairs[i][0], 128), ladder(lp, pairs[i][1], 128));
    if (!same_point(got, want)) fail("xyzz_mul_glv (arbitrary pair)", i);
  }
  Affine<F> id;
  memset(&id, 0, sizeof id);
  if (!xyzz_is_identity(glv_pair(id, low_half(ones), low_half(from_u64(5))))) fail("xyzz_mul_glv (identity input)", 0);
}

// the generators, Montgomery form (the constants of the Zcash specification)
static const u32 G1X[12] = {0xfd530c16u, 0x5cb38790u, 0x9976fff5u, 0x7817fc67u, 0x143ba1c1u, 0x154f95c7u,
                            0xf3d0e747u, 0xf0ae6acdu, 0x21dbf440u, 0xedce6eccu, 0x9e0bfb75u, 0x12017741u};
static const u32 G1Y[12] = {0x0ce72271u, 0xbaac93d5u, 0x7918fd8eu, 0x8c22631au, 0x570725ceu, 0xdd595f13u,
                            0x50405194u, 0x51ac5829u, 0xad0059c0u, 0x0e1c8c3fu, 0x5008a26au, 0x0bbc3efcu};
static void fp_from_hex(fp_t &r, const char *hex) {   // 96 hex digits, big-endian, canonical -> Montgomery
  fp_t c;
  for (int i = 0; i < 12; i++) {
    u32 w = 0;
    for (int d = 0; d < 8; d++) {
      const char ch = hex[(11 - i) * 8 + d];
      w = (w << 4) | (u32)(ch <= '9' ? ch - '0' : ch - 'a' + 10);
    }
    c.l[i] = w;
  }
  fe_to_mont(r, c);
}

int main() {
  U256 lambda{};
  for (int i = 0; i < 4; i++) lambda.l[i] = GlvConsts::lambda(i);
  const U256 one = from_u64(1), lam2 = mul(lambda, lambda), q1 = add(lam2, lambda);   // q - 1 = lambda (lambda + 1)
  std::vector<U256> corners = {from_u64(0), one, from_u64(2), sub(lambda, one), lambda, add(lambda, one),
                               sub(add(lambda, lambda), one), add(lambda, lambda), sub(lam2, one), lam2, sub(q1, one), q1,
                               shl(one, 127), sub(shl(one, 128), one), shl(one, 128), shl(one, 254)};
  const U256 ms[] = {from_u64(2), shl(one, 64), sub(lambda, one), add(lambda, one)};
  for (const U256 &m : ms) {
    const U256 ml = mul(m, lambda);
    for (const U256 &k : {sub(ml, one), ml, add(ml, one)})
      if (!less(q1, k)) corners.push_back(k);
  }
  std::vector<U256> scalars = corners;
  for (int it = 0; it < 10000; it++) {
    U256 k;
    for (int i = 0; i < 8; i += 2) {
      const uint64_t v = splitmix();
      k.l[i] = (u32)v;
      k.l[i + 1] = (u32)(v >> 32);
    }
    k.l[7] &= 0x3fffffffu;   // below 2^254 < q
    scalars.push_back(k);
  }
  for (size_t i = 0; i < scalars.size(); i++) {
    fr_t k;
    memcpy(&k, &scalars[i], sizeof k);
    glv_half k1, k2;
    glv_split(k, k1, k2);
    const U256 back = add(widen(k1), mul(widen(k2), lambda));
    if (memcmp(&back, &scalars[i], sizeof back) != 0 || !less(widen(k1), lambda)) fail("glv_split", i);
  }

  Affine<FpOps> g1;
  for (int i = 0; i < 12; i++) {
    g1.x.l[i] = G1X[i];
    g1.y.l[i] = G1Y[i];
  }
  Affine<Fp2Ops> g2;
  fp_from_hex(g2.x.c0, "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8");
  fp_from_hex(g2.x.c1, "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e");
  fp_from_hex(g2.y.c0, "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801");
  fp_from_hex(g2.y.c1, "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be");
  if (!on_curve(g1) || !on_curve(g2)) fail("generator", 0);
  std::vector<U256> some(corners);
  some.insert(some.end(), scalars.begin() + corners.size(), scalars.begin() + corners.size() + 12);
  check_ladder<FpOps>(g1, some, lambda);
  check_ladder<Fp2Ops>(g2, some, lambda);
  printf(bad ? "FAILED %d\n" : "glv host check: ok\n", bad);
  return bad ? 1 : 0;
}
