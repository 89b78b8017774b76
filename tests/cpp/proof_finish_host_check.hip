// Host check of the device proof assembly (bellman_amd/csrc/proof_finish.cuh) in a program of its own, so that it can run
// under ASan + UBSan without Python: finish_proof_host - the two stages the kernels of proof_finish.hip run, lane by lane -
// over corner and random rows against prover.rs:326-360 computed with the plain double-and-add ladder and the general
// addition.  The field and curve code is __host__ __device__: nothing here runs on a device.  Built and run by
// tests/test_proof_finish_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bellman_amd/csrc/proof_finish.cuh"

using namespace bh;

static uint64_t sm_state = 0x243F6A8885A308D3ull;
static uint64_t splitmix() {
  uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fr_t small_fr(uint64_t v) {   // canonical
  fr_t k{};
  k.l[0] = (u32)v;
  k.l[1] = (u32)(v >> 32);
  return k;
}
static fr_t random_fr() {   // canonical, below 2^254 < q
  fr_t k;
  for (int i = 0; i < 8; i += 2) {
    const uint64_t v = splitmix();
    k.l[i] = (u32)v;
    k.l[i + 1] = (u32)(v >> 32);
  }
  k.l[7] &= 0x3fffffffu;
  return k;
}
static fr_t q_minus_1() {
  fr_t r;
  for (int i = 0; i < 8; i++) r.l[i] = FrParams::mod(i);
  r.l[0] -= 1;   // q is odd
  return r;
}

static int bad = 0;
static void fail(const char *what, size_t i) {
  if (bad++ < 10) printf("%s fails at row %zu\n", what, i);
}

// (the force-inlined curve code is instantiated once per helper, not once per call: the build under sanitizers stays short)
template <class F>
__attribute__((noinline)) static XYZZ<F> ladder(const Affine<F> &p, const fr_t &k) {   // k canonical
  XYZZ<F> acc, px;
  xyzz_set_identity(acc);
  xyzz_from_affine(px, p);
  for (int i = 254; i >= 0; i--) {
    xyzz_dbl(acc, acc);
    if ((k.l[i >> 5] >> (i & 31)) & 1u) xyzz_add(acc, acc, px);
  }
  return acc;
}
template <class F>
__attribute__((noinline)) static XYZZ<F> plus(const XYZZ<F> &a, const XYZZ<F> &b) {
  XYZZ<F> r;
  xyzz_add(r, a, b);
  return r;
}
template <class F>
__attribute__((noinline)) static Affine<F> to_affine(const XYZZ<F> &p) {
  Affine<F> a;
  xyzz_to_affine(a, p);
  return a;
}
template <class F>
static XYZZ<F> lift(const Affine<F> &p) {
  XYZZ<F> x;
  xyzz_from_affine(x, p);
  return x;
}
template <class F>
static Affine<F> multiple(const Affine<F> &gen, const fr_t &k) {
  return to_affine(ladder(gen, k));
}
template <class F>
static Affine<F> negated(const Affine<F> &p) {
  Affine<F> r = p;
  if (!aff_is_identity(p)) {
    F::neg(r.y, p.y);
    F::canon(r.y);
  }
  return r;
}
__attribute__((noinline)) static FinishProof assemble(const FinishKey &key, const FinishSums &m, const fr_t &r, const fr_t &s) {
  fr_t rm, sm, rsm, rs;
  fe_to_mont(rm, r);
  fe_to_mont(sm, s);
  fe_mul(rsm, rm, sm);
  fe_from_mont(rs, rsm);
  FinishProof p;
  const XYZZ<FpOps> a_ans = plus(lift(m.a_in), lift(m.a_aux)), b1_ans = plus(lift(m.b1_in), lift(m.b1_aux));
  p.a = to_affine(plus(plus(ladder(key.delta_g1, r), lift(key.alpha_g1)), a_ans));                          // prover.rs:326-327, 339-343
  p.b = to_affine(plus(plus(ladder(key.delta_g2, s), lift(key.beta_g2)), plus(lift(m.b2_in), lift(m.b2_aux))));   // :328-329, 347-350
  XYZZ<FpOps> c = plus(plus(ladder(key.delta_g1, rs), ladder(key.alpha_g1, s)), ladder(key.beta_g1, r));   // :331-338
  c = plus(plus(c, ladder(to_affine(a_ans), s)), ladder(to_affine(b1_ans), r));                             // :342, 351-352
  p.c = to_affine(plus(plus(c, lift(m.h)), lift(m.l)));                                                     // :353-354
  return p;
}
__attribute__((noinline)) static FinishProof finish(const FinishKey &key, const FinishSums &m, const fr_t &r, const fr_t &s) {
  fr_t rm, sm;
  fe_to_mont(rm, r);
  fe_to_mont(sm, s);
  FinishProof p;
  finish_proof_host(p, key, m, rm, sm);
  return p;
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

struct Row {
  FinishSums m;
  fr_t r, s;
};

int main() {
  pf_g1 g1;
  for (int i = 0; i < 12; i++) {
    g1.x.l[i] = G1X[i];
    g1.y.l[i] = G1Y[i];
  }
  pf_g2 g2;
  fp_from_hex(g2.x.c0, "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8");
  fp_from_hex(g2.x.c1, "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e");
  fp_from_hex(g2.y.c0, "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801");
  fp_from_hex(g2.y.c1, "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be");
  if (!on_curve(g1) || !on_curve(g2)) fail("generator", 0);

  FinishKey key;
  key.alpha_g1 = multiple(g1, small_fr(18));
  key.beta_g1 = multiple(g1, small_fr(25));
  key.beta_g2 = multiple(g2, small_fr(30));
  key.delta_g1 = multiple(g1, small_fr(42));
  key.delta_g2 = multiple(g2, small_fr(47));

  auto random_sums = [&] {
    FinishSums m;
    pf_g1 *p1[6] = {&m.a_in, &m.a_aux, &m.b1_in, &m.b1_aux, &m.h, &m.l};
    for (pf_g1 *p : p1) *p = multiple(g1, small_fr(splitmix() >> 8));
    m.b2_in = multiple(g2, small_fr(splitmix() >> 8));
    m.b2_aux = multiple(g2, small_fr(splitmix() >> 8));
    return m;
  };
  std::vector<Row> rows;
  const FinishSums base = random_sums();
  FinishSums none;
  memset(&none, 0, sizeof none);
  rows.push_back(Row{base, random_fr(), random_fr()});
  rows.push_back(Row{random_sums(), small_fr(0), random_fr()});    // r = 0
  rows.push_back(Row{base, random_fr(), small_fr(0)});             // s = 0
  rows.push_back(Row{base, small_fr(0), small_fr(0)});
  rows.push_back(Row{base, q_minus_1(), small_fr(1)});
  rows.push_back(Row{none, random_fr(), random_fr()});             // every sum the identity
  {
    Row w{base, small_fr(7), small_fr(3)};
    w.m.a_aux = w.m.a_in;                                          // the doubling branch
    w.m.b2_aux = w.m.b2_in;
    rows.push_back(w);
    w.m.a_aux = negated(w.m.a_in);                                 // opposite points
    w.m.l = negated(w.m.h);
    rows.push_back(w);
  }
  for (int which = 0; which < 4; which++) {
    // ONE identity among an element's sums (two in a row would hide a missing identity case: adding the all-zero record
    // as if it were a point is an involution on the running sum)
    Row w{base, random_fr(), random_fr()};
    if (which == 0) memset(&w.m.a_aux, 0, sizeof w.m.a_aux);
    if (which == 1) memset(&w.m.b2_in, 0, sizeof w.m.b2_in);
    if (which == 2) memset(&w.m.h, 0, sizeof w.m.h);
    if (which == 3) memset(&w.m.b1_in, 0, sizeof w.m.b1_in);
    rows.push_back(w);
  }
  {
    // A and B the identity: a_in = -(alpha + [r] delta1), b2_in = -(beta2 + [s] delta2), the aux halves the identity
    Row w{base, small_fr(5), small_fr(9)};
    w.m.a_in = negated(to_affine(plus(ladder(key.delta_g1, w.r), lift(key.alpha_g1))));
    w.m.b2_in = negated(to_affine(plus(ladder(key.delta_g2, w.s), lift(key.beta_g2))));
    memset(&w.m.a_aux, 0, sizeof w.m.a_aux);
    memset(&w.m.b2_aux, 0, sizeof w.m.b2_aux);
    rows.push_back(w);
    const FinishProof p = finish(key, w.m, w.r, w.s);
    if (!aff_is_identity(p.a) || !aff_is_identity(p.b) || aff_is_identity(p.c)) fail("identity elements", rows.size() - 1);
  }
  for (size_t i = 0; i < rows.size(); i++) {
    const FinishProof got = finish(key, rows[i].m, rows[i].r, rows[i].s), want = assemble(key, rows[i].m, rows[i].r, rows[i].s);
    if (memcmp(&got.a, &want.a, sizeof got.a) != 0) fail("A", i);
    if (memcmp(&got.b, &want.b, sizeof got.b) != 0) fail("B", i);
    if (memcmp(&got.c, &want.c, sizeof got.c) != 0) fail("C", i);
  }
  printf(bad ? "FAILED %d\n" : "proof finish host check: ok\n", bad);
  return bad ? 1 : 0;
}
