// Groth16 verification on the device: prepare_verifying_key, verify_proof (groth16/src/verifier.rs:11-58) and the batch
// verifier (groth16/src/verifier/batch.rs:93-275), declared in include/bellman_hip.h.
//
// Device work per call (fp12.cuh holds the arithmetic and its conventions):
//   1. g2_lines_kernel      one lane per G2 point Q: the 68 projective line coefficients of the Miller loop over |x|
//                           ("G2Prepared"), written to HBM (288 B per line); the on-curve test of Q.
//   2. proof_prep_kernel    one lane per proof: the on-curve tests of A and C, A' = [z_j] A (double-and-add, one
//                           inversion to affine), C and z_j copied out as the bases / scalars of the sum of z_j C_j.
//   3. fr_colsum_kernels    acc_Gamma_i = sum_j z_j a_{j,i} (acc_Gamma_0 = acc_Y = sum_j z_j), Montgomery Fr.
//   4. miller_kernel        one lane per (P, lines of Q) pair: f = f_{|x|,Q}(P) in Fp12 (576 B).
//   5. f12_fold_kernel      the product of all f (a halving tree, one launch per level).
//   6. final_exp.cuh        one lane: f^(3 (p^12 - 1) / q) == 1, as a chain of small kernels.
// The two multiexps (sum z_j C_j over the proofs' C, Psi = sum acc_Gamma_i ic_i over the key's registered ic) run on
// the existing multiexp path (bh_msm_async_dev_after), ordered after the kernels that produce their inputs.
//
// Batches are processed in chunks of at most BATCH_CHUNK proofs (device workspace < 400 MB whatever the batch size); the
// Fp12 product of each chunk is folded into a running product that the next chunk multiplies in.
//
// Per-proof verdicts (bh_groth16_verify_each: Item::verify_single, batch.rs:55-66, for every proof of a batch) take one
// lane per proof through kernels 6-9 below instead of the multiexps and the product tree: ic_table_kernel (once per key),
// ic_accumulate_kernel, miller3_kernel, f12_mul_const_kernel, the same final exponentiation chain over the whole chunk,
// verdict_kernel.
//
// The host half: every call opens a CallFrame (device, pool buffers, a stream of its own).  The two walks over a batch,
// verify_each and batch_verify, are written once over a key policy - OneKey (a bh_pvk: the one-key kernels, rows taken
// from the caller's memory in the caller's order) or SetKeys (a bh_pvk_set: the key-aware kernels, rows grouped by key on
// the host) - which supplies what differs: where a chunk's rows come from (ChunkRows), the stage launches, the keys the
// tail loops over.  ProofChunk is the device side of a chunk's proofs (records, or bytes and Proof::read), chunk_rows the
// chunk size, finish_product the end of every pairing check.
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "pairing_kernels.cuh"

namespace bh {

// device buffers from the context's pool, returned on scope exit
struct PoolBufs {
  Context &c;
  std::vector<void *> held;
  explicit PoolBufs(Context &c_) : c(c_) {}
  ~PoolBufs() {
    for (void *p : held) c.pool.release(p);
  }
  template <class T>
  T *get(size_t n) {
    void *p = c.pool.acquire(n * sizeof(T));
    if (!p) return nullptr;
    held.push_back(p);
    return (T *)p;
  }
};
struct StreamHold {
  bh_ctx *ctx;
  hipStream_t st = nullptr;
  explicit StreamHold(bh_ctx *c) : ctx(c) {}
  ~StreamHold() {
    if (st) {
      (void)hipStreamSynchronize(st);
      bh_stream_destroy(ctx, (void *)st);
    }
  }
};

}  // namespace bh

using namespace bh;

// PreparedVerifyingKey (groth16/src/lib.rs:400-409): the lines of -gamma, -delta and beta in HBM, -alpha, and ic
// registered as multiexp bases (an identity ic_i is replaced by the generator and its scalar forced to zero)
struct bh_pvk {
  bh_ctx *ctx = nullptr;
  Affine<FpOps> neg_alpha;   // host, canonical Montgomery
  Affine<FpOps> alpha;
  line_t *lines = nullptr;   // [3][68]: -gamma, -delta, beta
  u32 *qflags = nullptr;     // [3]
  Affine<FpOps> *alpha_dev = nullptr;
  bh_bases *ic = nullptr;
  size_t n_ic = 0;
  std::vector<uint8_t> ic_identity;
  std::vector<Affine<FpOps>> ic_pts;   // ic as given (identities as they came)
  // What bh_groth16_verify_each adds to the key, built by the first call that needs it (std::call_once: the key is shared
  // const between threads): the window table of ic_1 .. ic_n, ic_0, and f(-alpha, beta).
  struct Each {
    std::once_flag once;
    int rc = BH_ERR_HIP;
    Affine<FpOps> *table = nullptr;   // [n_inputs][256 / w][2^w - 1]
    u32 w = 0;
    size_t table_bytes = 0;           // counted in the context's table budget (a bh_ctx_trim zeroes the context's count:
                                      // the release clamps)
    Affine<FpOps> *ic0 = nullptr;     // ic_0, then (inside the same block) the Fp12 constant
    fp12_t *f_ab = nullptr;
  };
  mutable Each each;
};

namespace {
// the generator of G1 (Montgomery form), from its canonical coordinates
void g1_generator(Affine<FpOps> &g) {
  static const u32 gx[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                             0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};
  static const u32 gy[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                             0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
  fp_t x, y;
  memcpy(x.l, gx, 48);
  memcpy(y.l, gy, 48);
  fe_to_mont(g.x, x);
  fe_to_mont(g.y, y);
}
void neg_g1_host(Affine<FpOps> &r, const Affine<FpOps> &a) {
  r = a;
  if (FpOps::is_zero_canonical(a.x, a.y)) return;
  bool zero = true;
  for (int i = 0; i < 12; i++) zero = zero && a.y.l[i] == 0;
  if (zero) return;
  u32 br = 0;
  for (int i = 0; i < 12; i++) r.y.l[i] = subb(FpParams::mod(i), a.y.l[i], br, br);
}
// a 32-byte little-endian value that is 0 mod q: 0, q or 2q (3q > 2^256); the same test holds for a Montgomery
// representative, as aR = 0 mod q exactly when a = 0 mod q
bool scalar_is_zero_mod_q(const uint8_t *s) {
  u32 w[8];
  memcpy(w, s, 32);
  bool zero = true, is_q = true, is_2q = true;
  u32 carry = 0;
  for (int i = 0; i < 8; i++) {
    const u32 m = FrParams::mod(i);
    const u32 m2 = (m << 1) | carry;
    carry = m >> 31;
    zero = zero && w[i] == 0;
    is_q = is_q && w[i] == m;
    is_2q = is_2q && w[i] == m2;
  }
  return zero || is_q || is_2q;
}

// What a call holds on the device: the context's device made current, buffers from the pool and a stream of the call's
// own (rc says whether it got them).  bufs is declared before the stream: released only after the stream has drained.
struct CallFrame {
  PoolBufs bufs;
  StreamHold sh;
  hipStream_t st = nullptr;
  int rc;
  explicit CallFrame(bh_ctx *ctx) : bufs(ctx->c), sh(ctx), rc(open(ctx)) {}

 private:
  int open(bh_ctx *ctx) {
    BH_HIP_CHECK(hipSetDevice(ctx->c.device));
    if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) {
      sh.st = nullptr;
      return BH_ERR_HIP;
    }
    st = sh.st;
    return BH_OK;
  }
};

// proof_prep_kernel over m proofs; zd .. gen are NULL where only the curve tests and A are wanted (verdicts, verify_proof)
int launch_proof_prep(hipStream_t st, const ProofRec *pr, const fr_t *zd, int fmt, Affine<FpOps> *pts, Affine<FpOps> *cb, fr_t *zc,
                      const Affine<FpOps> *gen, u32 *pflags, size_t m) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(proof_prep_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, pr, zd, fmt, pts, cb, zc, gen, pflags, (u32)m);
  return hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
}

// The end of every pairing check: fk holds n Miller values, then room for one more and 5 values of workspace.  Their
// product - times facc, the proofs' product so far, unless NULL - goes through the final exponentiation; *is_one is
// valid on return (the stream is synchronised).
int finish_product(hipStream_t st, fp12_t *fk, size_t n, const fp12_t *facc, u32 *is_one_dev, bool *is_one) {
  fp12_t *fe = fk + n + 1;
  if (facc) {
    if (hipMemcpyAsync(fk + n, facc, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return BH_ERR_HIP;
    n++;
  }
  int rc = launch_fold(st, fk, n);
  if (rc) return rc;
  if ((rc = launch_final_exp(st, fk, 1, fe, is_one_dev, fe + 1))) return rc;
  u32 h = 0;
  if (hipMemcpyAsync(&h, is_one_dev, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return BH_ERR_HIP;
  *is_one = h == 1;
  return BH_OK;
}
// verify_proof's pairing check: n_own pairs of the caller's (P at key_p_dev - n_own, lines own_lines) and the three key
// pairs (key_p_dev: the G1 points paired with -gamma, -delta, beta) in one Miller launch, then finish_product
int finish_check(hipStream_t st, const bh_pvk *pvk, PoolBufs &bufs, const Affine<FpOps> *key_p_dev, size_t n_own,
                 const line_t *own_lines, const u32 *own_flags, u32 *is_one_dev, bool *is_one) {
  fp12_t *fk = bufs.get<fp12_t>(n_own + 3 + 1 + 5);
  if (!fk) return BH_ERR_HIP;
  const int rc = launch_miller(st, key_p_dev - n_own, own_lines, own_flags, fk, n_own, pvk->lines, pvk->qflags, 3);
  if (rc) return rc;
  return finish_product(st, fk, n_own + 3, nullptr, is_one_dev, is_one);
}
}  // namespace

extern "C" {

int bh_groth16_prepare_verifying_key(bh_ctx *ctx, const void *alpha_g1, const void *beta_g2, const void *gamma_g2,
                                     const void *delta_g2, const void *ic, size_t n_ic, bh_pvk **out) {
  if (!ctx || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !out || (n_ic && !ic) || !n_ic) return BH_ERR_INVALID_ARG;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  std::unique_ptr<bh_pvk> k(new bh_pvk);
  k->ctx = ctx;
  memcpy(&k->alpha, alpha_g1, 96);
  neg_g1_host(k->neg_alpha, k->alpha);
  k->n_ic = n_ic;
  // ic with identities replaced by the generator (their scalars are zeroed at use)
  std::vector<Affine<FpOps>> icv(n_ic);
  memcpy(icv.data(), ic, n_ic * 96);
  k->ic_pts = icv;
  Affine<FpOps> gen;
  g1_generator(gen);
  k->ic_identity.assign(n_ic, 0);
  for (size_t i = 0; i < n_ic; i++)
    if (FpOps::is_zero_canonical(icv[i].x, icv[i].y)) {
      k->ic_identity[i] = 1;
      icv[i] = gen;
    }
  int rc = bh_bases_register(ctx, BH_G1, icv.data(), n_ic, 96, -1, &k->ic);
  if (rc) return rc;
  k->lines = (line_t *)c.pool.acquire(3 * MILLER_LINES * sizeof(line_t));
  k->qflags = (u32 *)c.pool.acquire(3 * sizeof(u32) + 2 * sizeof(Affine<FpOps>));
  if (!k->lines || !k->qflags) {
    bh_groth16_pvk_release(k.release());
    return BH_ERR_HIP;
  }
  k->alpha_dev = (Affine<FpOps> *)((char *)k->qflags + 64);
  // -gamma, -delta, beta (groth16/src/verifier.rs:11-21) and their lines
  std::vector<Affine<Fp2Ops>> q(3);
  memcpy(&q[0], gamma_g2, 192);
  memcpy(&q[1], delta_g2, 192);
  memcpy(&q[2], beta_g2, 192);
  void *qd = c.pool.acquire(3 * 192);
  if (!qd) {
    bh_groth16_pvk_release(k.release());
    return BH_ERR_HIP;
  }
  hipStream_t st = c.stream;
  std::vector<u32> fl(3, 0);
  rc = BH_OK;
  if (hipMemcpyAsync(qd, q.data(), 3 * 192, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(k->alpha_dev, &k->alpha, 96, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = BH_ERR_HIP;
  if (!rc) rc = launch_g2_lines(st, qd, 192, 1, k->lines, k->qflags, 2);                 // -gamma, -delta
  if (!rc) rc = launch_g2_lines(st, (char *)qd + 2 * 192, 192, 0, k->lines + 2 * MILLER_LINES, k->qflags + 2, 1);   // beta
  if (!rc && hipMemcpyAsync(fl.data(), k->qflags, 12, hipMemcpyDeviceToHost, st) != hipSuccess) rc = BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
  c.pool.release(qd);
  if (!rc)
    for (u32 f : fl)
      if (f & PF_OFF_CURVE) rc = BH_ERR_INVALID_POINT;
  if (rc) {
    bh_groth16_pvk_release(k.release());
    return rc;
  }
  *out = k.release();
  return BH_OK;
}

void bh_groth16_pvk_release(bh_pvk *pvk) {
  if (!pvk) return;
  Context &c = pvk->ctx->c;
  (void)hipSetDevice(c.device);
  if (pvk->ic) bh_bases_release(pvk->ctx, pvk->ic);
  c.pool.release(pvk->each.table);
  c.pool.release(pvk->each.ic0);
  if (pvk->each.table_bytes) {
    std::lock_guard<std::mutex> g(c.job_mu);
    c.table_bytes = c.table_bytes > pvk->each.table_bytes ? c.table_bytes - pvk->each.table_bytes : 0;
  }
  c.pool.release(pvk->lines);
  c.pool.release(pvk->qflags);
  delete pvk;
}

size_t bh_groth16_pvk_num_inputs(const bh_pvk *pvk) { return pvk ? pvk->n_ic - 1 : 0; }

// verify_proof (groth16/src/verifier.rs:23-58): acc = ic_0 + sum inputs_i ic_{i+1} (a multiexp over the registered ic),
// then e(A, B) e(acc, -gamma) e(C, -delta) e(-alpha, beta) == 1 with one final exponentiation - the reference compares
// the first three against e(alpha, beta), the same equation.
int bh_groth16_verify(const bh_pvk *pvk, const void *proof, const void *inputs, size_t n_inputs, int scalar_fmt) {
  if (!pvk || !proof || (n_inputs && !inputs) || (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT))
    return BH_ERR_INVALID_ARG;
  if (n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;   // verifier.rs:27-29
  bh_ctx *ctx = pvk->ctx;
  CallFrame fr(ctx);
  if (fr.rc) return fr.rc;
  hipStream_t st = fr.st;
  // scalars [1, inputs...] over ic
  std::vector<uint8_t> sc(32 * pvk->n_ic, 0);
  if (scalar_fmt == BH_SCALARS_MONT) {
    for (int i = 0; i < 8; i++) {
      const u32 w = FrParams::one(i);
      memcpy(&sc[4 * i], &w, 4);
    }
  } else {
    sc[0] = 1;
  }
  if (n_inputs) memcpy(&sc[32], inputs, 32 * n_inputs);
  for (size_t i = 0; i < pvk->n_ic; i++)
    if (pvk->ic_identity[i]) memset(&sc[32 * i], 0, 32);
  bh_msm_job *job = nullptr;
  int rc = bh_msm_async(ctx, pvk->ic, 0, sc.data(), pvk->n_ic, scalar_fmt, nullptr, 0, &job);
  if (rc) return rc;
  ProofRec *pr = fr.bufs.get<ProofRec>(1);
  Affine<FpOps> *pts = fr.bufs.get<Affine<FpOps>>(4);   // [A, acc, C, -alpha]
  line_t *lines = fr.bufs.get<line_t>(MILLER_LINES);
  u32 *flags = fr.bufs.get<u32>(4);
  Affine<FpOps> acc;
  Affine<FpOps> key[3];   // source of an asynchronous copy: lives until finish_check has synchronised
  if (!pr || !pts || !lines || !flags) {
    bh_msm_wait(job, &acc);
    return BH_ERR_HIP;
  }
  const ProofRec *hp = (const ProofRec *)proof;
  if (hipMemcpyAsync(pr, proof, sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
  if (!rc) rc = launch_proof_prep(st, pr, nullptr, 0, pts, nullptr, nullptr, nullptr, flags, 1);
  if (!rc) rc = launch_g2_lines(st, &pr->b, sizeof(ProofRec), 0, lines, flags + 1, 1);
  const int mrc = bh_msm_wait(job, &acc);
  if (!rc) rc = mrc;
  if (!rc) {
    key[0] = acc;
    key[1] = hp->c;
    key[2] = pvk->neg_alpha;
    if (hipMemcpyAsync(pts + 1, key, sizeof key, hipMemcpyHostToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
  }
  bool one = false;
  if (!rc) rc = finish_check(st, pvk, fr.bufs, pts + 1, 1, lines, flags + 1, flags + 3, &one);
  u32 hf[2] = {0, 0};
  if (!rc && (hipMemcpyAsync(hf, flags, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
    rc = BH_ERR_HIP;
  if (rc) return rc;
  if ((hf[0] | hf[1]) & PF_OFF_CURVE) return BH_ERR_INVALID_POINT;
  return one ? BH_OK : BH_ERR_INVALID_PROOF;
}

}  // extern "C"

// ---- proofs of several keys in one call --------------------------------------------------------------------------------
// A bh_pvk_set names 1 .. BH_PVK_SET_MAX_KEYS prepared keys of one context and owns one device table of KeyDesc
// (pairing_kernels.cuh).  The half of a descriptor that the batch check reads (lines, flags, alpha, input count, column
// offset) is written when the set is made; the half that verify_each adds to a key (bh_pvk::Each: window table, width,
// ic_0, f(-alpha, beta)) is built key by key through the key's own std::call_once and written into a second copy of the
// table by the first bh_groth16_verify_each_keys* call.  Neither copy changes after it is written.
// Every chunk is grouped by key on the host (a stable counting sort) and cut into blocks of at most 64 rows of one key;
// proofs, inputs and z go up in that order, verdicts and status words come back through the permutation.
struct bh_pvk_set {
  bh_ctx *ctx = nullptr;
  std::vector<const bh_pvk *> keys;
  std::vector<KeyDesc> host;      // the descriptors as uploaded at creation
  KeyDesc *dev = nullptr;         // [2][n_keys]: the batch's copy, then verify_each's
  size_t total_cols = 0, max_in = 0;
  mutable std::once_flag each_once;
  mutable int each_rc = BH_ERR_HIP;
};

namespace {
// verify_each's share of a key, once per key: the largest window of 8, 4, 2, 1 bits whose table fits the context's table
// budget, ic_0 and f(-alpha, beta)
void build_each(const bh_pvk *pvk) {
  bh_pvk::Each &e = pvk->each;
  Context &c = pvk->ctx->c;
  const size_t n_in = pvk->n_ic - 1;
  e.rc = BH_ERR_HIP;
  CallFrame fr(pvk->ctx);
  if (fr.rc) return;
  hipStream_t st = fr.st;
  for (u32 w = 8; n_in && w >= 1; w >>= 1) {
    const size_t bytes = n_in * (256 / w) * ((size_t(1) << w) - 1) * sizeof(Affine<FpOps>);
    {
      std::lock_guard<std::mutex> g(c.job_mu);
      if (w > 1 && c.table_bytes + bytes > c.table_budget) continue;   // (one-bit windows are the floor)
      c.table_bytes += bytes;
    }
    e.table = (Affine<FpOps> *)c.pool.acquire(bytes);
    if (e.table) {
      e.w = w;
      e.table_bytes = bytes;
      break;
    }
    std::lock_guard<std::mutex> g(c.job_mu);
    c.table_bytes -= bytes;
  }
  if (n_in && !e.table) {
    fprintf(stderr, "[bellman_hip] verify_each: no device memory for the window table of %zu ic points\n", n_in);
    return;
  }
  e.ic0 = (Affine<FpOps> *)c.pool.acquire(sizeof(Affine<FpOps>) + 32 + sizeof(fp12_t) + sizeof(Affine<FpOps>));
  Affine<FpOps> *icd = fr.bufs.get<Affine<FpOps>>(pvk->n_ic);
  if (!e.ic0 || !icd) return;
  e.f_ab = (fp12_t *)((char *)e.ic0 + 128);
  Affine<FpOps> *na = (Affine<FpOps> *)(e.f_ab + 1);
  bool ok = hipMemcpyAsync(icd, pvk->ic_pts.data(), pvk->n_ic * sizeof(Affine<FpOps>), hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(e.ic0, pvk->ic_pts.data(), sizeof(Affine<FpOps>), hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(na, &pvk->neg_alpha, sizeof(Affine<FpOps>), hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok && n_in) {
    const size_t total = e.table_bytes / sizeof(Affine<FpOps>);
    (void)hipGetLastError();
    hipLaunchKernelGGL(ic_table_kernel, dim3(blocks_of(total, 64)), dim3(64), 0, st, icd + 1, e.w, e.table, (u32)total);
    ok = hipGetLastError() == hipSuccess;
  }
  // f(-alpha, beta): one lane of the existing Miller kernel over the key's beta lines
  if (ok) ok = launch_miller(st, na, pvk->lines + 2 * MILLER_LINES, pvk->qflags + 2, e.f_ab, 1) == BH_OK;
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  if (ok) e.rc = BH_OK;
}

void set_build_each(const bh_pvk_set *set) {
  std::vector<KeyDesc> d = set->host;
  for (size_t k = 0; k < d.size(); k++) {
    const bh_pvk *pvk = set->keys[k];
    std::call_once(pvk->each.once, build_each, pvk);
    if (pvk->each.rc) {
      set->each_rc = pvk->each.rc;
      return;
    }
    d[k].table = pvk->each.table;
    d[k].w = pvk->each.w ? pvk->each.w : 8u;
    d[k].ic0 = pvk->each.ic0;
    d[k].f_ab = pvk->each.f_ab;
  }
  CallFrame fr(set->ctx);
  if (fr.rc) return;
  if (hipMemcpyAsync(set->dev + d.size(), d.data(), d.size() * sizeof(KeyDesc), hipMemcpyHostToDevice, fr.st) != hipSuccess ||
      hipStreamSynchronize(fr.st) != hipSuccess)
    return;
  set->each_rc = BH_OK;
}

// the rows [first, first + m) of a call grouped by key
struct Grouping {
  std::vector<u32> perm;          // grouped row r is the chunk's row perm[r]
  std::vector<KeySeg> segs;       // per key
  std::vector<KeyBlock> blocks;
  size_t n_in = 0, max_seg = 0;   // scalars of the chunk; its longest run
  void make(const bh_pvk_set *set, const uint32_t *key_of, size_t m) {
    const size_t nk = set->keys.size();
    segs.assign(nk, KeySeg{0, 0, 0, 0});
    for (size_t j = 0; j < m; j++) segs[key_of[j]].count++;
    u32 row = 0, in = 0;
    blocks.clear();
    max_seg = 0;
    for (size_t k = 0; k < nk; k++) {
      const u32 n_inputs = set->host[k].n_inputs;
      segs[k].first = row;
      segs[k].in_off = in;
      for (u32 t = 0; t < segs[k].count; t += 64)
        blocks.push_back(KeyBlock{(u32)k, row + t, std::min<u32>(64, segs[k].count - t), in + t * n_inputs});
      row += segs[k].count;
      in += segs[k].count * n_inputs;
      max_seg = std::max<size_t>(max_seg, segs[k].count);
    }
    n_in = in;
    perm.resize(m);
    std::vector<u32> next(nk);
    for (size_t k = 0; k < nk; k++) next[k] = segs[k].first;
    for (size_t j = 0; j < m; j++) perm[next[key_of[j]]++] = (u32)j;
  }
};

bool scalar_fmt_ok(int fmt) { return fmt == BH_SCALARS_CANONICAL || fmt == BH_SCALARS_MONT; }

// the chunk: at most BATCH_CHUNK proofs, and at most INPUTS_CHUNK_BYTES of public inputs if every proof had the widest
// input count of the call
size_t chunk_rows(size_t n_proofs, size_t widest_input_count) {
  const size_t by_inputs = std::max<size_t>(1, INPUTS_CHUNK_BYTES / (32 * std::max<size_t>(widest_input_count, 1)));
  return std::min(std::min(n_proofs, BATCH_CHUNK), by_inputs);
}

// The device side of a chunk's proofs, common to every walk: the affine records the kernels read and, for proofs given as
// bytes (Proof::write's 192 B each), the chunk as written, the reader's per-point status, its status word per proof and
// the first proof of the chunk that it refuses.
struct ProofChunk {
  bool compressed = false;
  ProofRec *pr = nullptr;
  unsigned char *cbytes = nullptr;
  u32 *pst = nullptr, *words = nullptr;   // words: NULL for records, which is what verdict_kernel expects then
  unsigned long long *first_bad = nullptr;
  bool alloc(PoolBufs &bufs, size_t ch, bool bytes) {
    compressed = bytes;
    pr = bufs.get<ProofRec>(ch);
    if (!bytes) return pr != nullptr;
    cbytes = bufs.get<unsigned char>(ch * 192);
    pst = bufs.get<u32>(4 * ch);
    first_bad = bufs.get<unsigned long long>(1);
    if (pst) words = pst + 3 * ch;
    return pr && cbytes && pst && first_bad;
  }
  // m rows from the host: records, or bytes that Proof::read decodes on the stream (every point checked, the identity
  // refused; a refused proof's points go on as identities).  reset_first_bad before the read for whoever reads first_bad;
  // read_back: where to download it right behind the read, or NULL.
  int upload(hipStream_t st, const void *rows, size_t m, bool reset_first_bad, unsigned long long *read_back) const {
    if (!compressed)
      return hipMemcpyAsync(pr, rows, m * sizeof(ProofRec), hipMemcpyHostToDevice, st) == hipSuccess ? BH_OK : BH_ERR_HIP;
    if (hipMemcpyAsync(cbytes, rows, m * 192, hipMemcpyHostToDevice, st) != hipSuccess ||
        (reset_first_bad && hipMemsetAsync(first_bad, 0xff, 8, st) != hipSuccess))
      return BH_ERR_HIP;
    const int rc = proofs_read_dev(cbytes, pr, m, pst, words, first_bad, st);
    if (rc) return rc;
    if (read_back && hipMemcpyAsync(read_back, first_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess) return BH_ERR_HIP;
    return BH_OK;
  }
};

// Where a chunk's rows are uploaded from, in the order the kernels see them.  perm: row r of that order is the chunk's
// row perm[r] in the caller's; NULL when the order IS the caller's and the pointers go straight into the caller's memory.
struct ChunkRows {
  const void *recs, *inputs, *z;   // z: NULL for verdicts
  size_t n_in;                     // scalars at inputs
  const u32 *perm;
};

// ---- the key policies: what differs between a call under one key and a call under a set ------------------------------------
// Both supply: the keys (count, key k, its first column in the column sums, its run of rows in a chunk), the input counts
// (widest, scalars in front of proof j), a chunk's rows, and the stage launches - accumulate, miller3 and fold3_const for
// verdicts; colsum, mul_alpha ([acc_Y] alpha) and miller_pairs (the key pairs) for the batch check.
struct OneKey {   // the one-key kernels; rows in the caller's order, uploaded from the caller's memory
  const bh_pvk *pvk;
  bh_ctx *ctx() const { return pvk->ctx; }
  size_t n_keys() const { return 1; }
  const bh_pvk *key(size_t) const { return pvk; }
  size_t col_off(size_t) const { return 0; }
  size_t total_cols() const { return pvk->n_ic; }
  size_t widest() const { return pvk->n_ic - 1; }
  size_t scalars_before(size_t j) const { return j * (pvk->n_ic - 1); }
  KeySeg run(size_t, size_t m) const { return KeySeg{0, (u32)m, 0, 0}; }
  ChunkRows rows(const void *src, size_t rec, const void *inputs, const void *z, size_t first, size_t m) {
    return ChunkRows{(const unsigned char *)src + first * rec, (const fr_t *)inputs + scalars_before(first),
                     z ? (const fr_t *)z + first : nullptr, scalars_before(m), nullptr};
  }
  int prepare_each() const {
    BH_HIP_CHECK(hipSetDevice(pvk->ctx->c.device));
    std::call_once(pvk->each.once, build_each, pvk);
    return pvk->each.rc;
  }
  bool alloc_each(PoolBufs &, size_t) { return true; }
  bool alloc_batch(PoolBufs &) { return true; }
  int upload_layout(hipStream_t, bool) const { return BH_OK; }
  int accumulate(hipStream_t st, const fr_t *ind, int fmt, Affine<FpOps> *out, size_t m) const {
    const bh_pvk::Each &e = pvk->each;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ic_accumulate_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, ind, (u32)(pvk->n_ic - 1), fmt, e.table,
                       e.w ? e.w : 8u, e.ic0, out, (u32)m);
    return hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  }
  int miller3(hipStream_t st, const Affine<FpOps> *a, const Affine<FpOps> *acc, const ProofRec *pr, const line_t *lines,
              const u32 *qflags, bool separate, fp12_t *f, size_t m) const {
    (void)hipGetLastError();
    hipLaunchKernelGGL(miller3_kernel, dim3(blocks_of(m, 64), separate ? 3 : 1), dim3(64), 0, st, a, acc, pr, lines, qflags,
                       pvk->lines, pvk->qflags, 7u, f, (u32)m);
    return hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  }
  int fold3_const(hipStream_t st, fp12_t *f, size_t m, bool separate) const {
    return launch_fold3_const(st, f, pvk->each.f_ab, m, separate);
  }
  int colsum(hipStream_t st, const fr_t *zd, const fr_t *ind, int fmt, size_t m, fr_t *part, fr_t *acc) const {
    return launch_colsum(st, zd, ind, pvk->n_ic - 1, fmt, m, part, acc);
  }
  int mul_alpha(hipStream_t st, Affine<FpOps> *out, const fr_t *acc) const {
    (void)hipGetLastError();
    hipLaunchKernelGGL(g1_mul_one_kernel, dim3(1), dim3(64), 0, st, out, pvk->alpha_dev, acc);
    return hipGetLastError() == hipSuccess ? BH_OK : BH_ERR_HIP;
  }
  int miller_pairs(hipStream_t st, const Affine<FpOps> *key, fp12_t *fk) const {
    return launch_miller(st, key, pvk->lines, pvk->qflags, fk, 3);
  }
};

struct SetKeys {   // the key-aware kernels; every chunk grouped by key on the host (Grouping), rows uploaded from that copy
  const bh_pvk_set *set = nullptr;
  const uint32_t *key_of = nullptr;
  std::vector<size_t> offs;   // offs[j]: the first scalar of proof j in the call's inputs (n_proofs + 1 values)
  Grouping g;                 // of the current chunk
  std::vector<unsigned char> hrec, hin, hz;
  KeyBlock *blk = nullptr;
  KeySeg *segd = nullptr;
  // the call-level checks both forms share
  int init(const bh_pvk_set *s, const uint32_t *ko, size_t n_proofs, const void *inputs, size_t n_inputs_total, int scalar_fmt) {
    if (!s || (n_proofs && !ko) || !scalar_fmt_ok(scalar_fmt)) return BH_ERR_INVALID_ARG;
    set = s;
    key_of = ko;
    const size_t nk = set->keys.size();
    offs.resize(n_proofs + 1);
    size_t total = 0;
    for (size_t j = 0; j < n_proofs; j++) {
      if (key_of[j] >= nk) return BH_ERR_INVALID_ARG;
      offs[j] = total;
      total += set->host[key_of[j]].n_inputs;
    }
    offs[n_proofs] = total;
    if (total != n_inputs_total) return BH_ERR_INVALID_VERIFYING_KEY;   // batch.rs:101-107, for every proof's own key
    if (total && !inputs) return BH_ERR_INVALID_ARG;
    return BH_OK;
  }
  bh_ctx *ctx() const { return set->ctx; }
  size_t n_keys() const { return set->keys.size(); }
  const bh_pvk *key(size_t k) const { return set->keys[k]; }
  size_t col_off(size_t k) const { return set->host[k].col_off; }
  size_t total_cols() const { return set->total_cols; }
  size_t widest() const { return set->max_in; }
  size_t scalars_before(size_t j) const { return offs[j]; }
  KeySeg run(size_t k, size_t) const { return g.segs[k]; }
  ChunkRows rows(const void *src, size_t rec, const void *inputs, const void *z, size_t first, size_t m) {
    g.make(set, key_of + first, m);
    hrec.resize(m * rec);
    hin.resize(std::max<size_t>(g.n_in, 1) * 32);
    hz.resize(z ? m * 32 : 0);
    size_t in = 0;
    for (size_t r = 0; r < m; r++) {
      const size_t j = first + g.perm[r];
      memcpy(&hrec[r * rec], (const unsigned char *)src + j * rec, rec);
      const size_t cnt = offs[j + 1] - offs[j];
      if (cnt) memcpy(&hin[in * 32], (const unsigned char *)inputs + offs[j] * 32, cnt * 32);
      in += cnt;
      if (z) memcpy(&hz[r * 32], (const unsigned char *)z + j * 32, 32);
    }
    return ChunkRows{hrec.data(), hin.data(), z ? hz.data() : nullptr, g.n_in, g.perm.data()};
  }
  int prepare_each() const {
    BH_HIP_CHECK(hipSetDevice(set->ctx->c.device));
    std::call_once(set->each_once, set_build_each, set);
    return set->each_rc;
  }
  bool alloc_each(PoolBufs &bufs, size_t ch) { return (blk = bufs.get<KeyBlock>(ch / 64 + n_keys() + 1)) != nullptr; }
  bool alloc_batch(PoolBufs &bufs) { return (segd = bufs.get<KeySeg>(n_keys())) != nullptr; }
  // the chunk's block table (verdicts) or per-key runs (the batch check), in front of its rows
  int upload_layout(hipStream_t st, bool each) const {
    const hipError_t e = each ? hipMemcpyAsync(blk, g.blocks.data(), g.blocks.size() * sizeof(KeyBlock), hipMemcpyHostToDevice, st)
                              : hipMemcpyAsync(segd, g.segs.data(), g.segs.size() * sizeof(KeySeg), hipMemcpyHostToDevice, st);
    return e == hipSuccess ? BH_OK : BH_ERR_HIP;
  }
  const KeyDesc *each_desc() const { return set->dev + n_keys(); }
  int accumulate(hipStream_t st, const fr_t *ind, int fmt, Affine<FpOps> *out, size_t) const {
    return launch_ic_accumulate_keys(st, ind, fmt, each_desc(), blk, g.blocks.size(), out);
  }
  int miller3(hipStream_t st, const Affine<FpOps> *a, const Affine<FpOps> *acc, const ProofRec *pr, const line_t *lines,
              const u32 *qflags, bool separate, fp12_t *f, size_t m) const {
    return launch_miller3_keys(st, a, acc, pr, lines, qflags, each_desc(), blk, g.blocks.size(), separate, f, m);
  }
  int fold3_const(hipStream_t st, fp12_t *f, size_t m, bool separate) const {
    return launch_fold3_const_keys(st, f, each_desc(), blk, g.blocks.size(), m, separate);
  }
  int colsum(hipStream_t st, const fr_t *zd, const fr_t *ind, int fmt, size_t, fr_t *part, fr_t *acc) const {
    return launch_colsum_keys(st, zd, ind, fmt, set->dev, segd, n_keys(), set->max_in + 1, set->total_cols, g.max_seg, part, acc);
  }
  int mul_alpha(hipStream_t st, Affine<FpOps> *out, const fr_t *acc) const {
    return launch_g1_mul_keys(st, out, set->dev, acc, n_keys());
  }
  int miller_pairs(hipStream_t st, const Affine<FpOps> *key, fp12_t *fk) const {
    return launch_miller_keys(st, key, set->dev, n_keys(), fk);
  }
};

// the call-level checks of the one-key forms; per_row: the verdicts or the z, one per proof
int one_key_check_args(const bh_pvk *pvk, const void *rows, const void *per_row, size_t n_proofs, const void *inputs,
                       size_t n_inputs, int scalar_fmt) {
  if (!pvk || (n_proofs && (!rows || !per_row)) || (n_proofs && n_inputs && !inputs) || !scalar_fmt_ok(scalar_fmt))
    return BH_ERR_INVALID_ARG;
  if (n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;   // verifier.rs:27-29, batch.rs:101-107
  return BH_OK;
}

// the most scalars any chunk of the call holds (at least 1: the buffer exists)
template <class Keys>
size_t most_scalars(const Keys &keys, size_t n_proofs, size_t ch) {
  size_t most = 1;
  for (size_t first = 0; first < n_proofs; first += ch)
    most = std::max(most, keys.scalars_before(std::min(first + ch, n_proofs)) - keys.scalars_before(first));
  return most;
}

// ---- per-proof verdicts: Item::verify_single for every proof of a batch (groth16/src/verifier/batch.rs:55-66, which is
// verify_proof, groth16/src/verifier.rs:23-58) in one call --------------------------------------------------------------
// Every proof takes one lane through: proof_prep_kernel / g2_lines_kernel (curve flags, B_j's lines), the ic accumulation
// (acc_j from its key's window table), the three-pair Miller loops (shared squarings or three one-pair loops), the
// product with its key's f(-alpha, beta), the n-wide final exponentiation chain and verdict_kernel.  No multiexp job, no
// host loop over proofs; one download and one synchronisation per chunk, straight into the caller's arrays unless the
// chunk's rows were permuted.  src: records, or bytes that each chunk decodes first; the arguments are checked.
template <class Keys>
int verify_each(Keys &keys, const void *src, bool compressed, size_t n_proofs, const void *inputs, int scalar_fmt,
                int32_t *verdicts, uint32_t *status, size_t *n_bad) {
  if (n_bad) *n_bad = 0;
  if (!n_proofs) return BH_OK;
  int rc = keys.prepare_each();
  if (rc) return rc;
  CallFrame fr(keys.ctx());
  if (fr.rc) return fr.rc;
  hipStream_t st = fr.st;
  PoolBufs &bufs = fr.bufs;
  const bool separate = !env().verify_each_shared;   // three one-pair loops: the faster form at 2^14 proofs, see miller3_kernel
  const size_t ch = chunk_rows(n_proofs, keys.widest());
  ProofChunk pc;
  const bool have_pc = pc.alloc(bufs, ch, compressed);
  fr_t *ind = bufs.get<fr_t>(most_scalars(keys, n_proofs, ch));
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(2 * ch);   // A_j, then acc_j
  line_t *lines = bufs.get<line_t>(ch * MILLER_LINES);
  u32 *words = bufs.get<u32>(4 * ch);                     // curve flags of A/C, of B, is_one, verdicts
  fp12_t *f = bufs.get<fp12_t>((separate ? 3 : 1) * ch);
  fp12_t *ws = bufs.get<fp12_t>(4 * ch);                  // final exponentiation workspace
  if (!have_pc || !ind || !pts || !lines || !words || !f || !ws || !keys.alloc_each(bufs, ch)) {
    fprintf(stderr, "[bellman_hip] verify_each: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  u32 *pflags = words, *qflags = words + ch, *is_one = words + 2 * ch;
  int *vd = (int *)(words + 3 * ch);
  Affine<FpOps> *accp = pts + ch;
  const size_t rec = compressed ? 192 : sizeof(ProofRec);
  std::vector<int32_t> hv;   // a permuted chunk's verdicts and status words
  std::vector<uint32_t> hs;
  size_t bad = 0;
  for (size_t first = 0; first < n_proofs; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    const ChunkRows o = keys.rows(src, rec, inputs, nullptr, first, m);
    if ((rc = keys.upload_layout(st, true))) return rc;
    if ((rc = pc.upload(st, o.recs, m, false, nullptr))) return rc;
    if (o.n_in && hipMemcpyAsync(ind, o.inputs, o.n_in * 32, hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
    if ((rc = launch_proof_prep(st, pc.pr, nullptr, 0, pts, nullptr, nullptr, nullptr, pflags, m))) return rc;
    if ((rc = keys.accumulate(st, ind, scalar_fmt, accp, m))) return rc;
    if ((rc = launch_g2_lines(st, &pc.pr->b, sizeof(ProofRec), 0, lines, qflags, m))) return rc;
    if ((rc = keys.miller3(st, pts, accp, pc.pr, lines, qflags, separate, f, m))) return rc;
    if ((rc = keys.fold3_const(st, f, m, separate))) return rc;
    if ((rc = launch_final_exp(st, f, m, f, is_one, ws))) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(verdict_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, st, pc.words, pflags, qflags, is_one, vd, (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    int32_t *v = verdicts + first;
    uint32_t *s = status ? status + first : nullptr;
    if (o.perm) {
      hv.resize(m);
      hs.resize(m);
      v = hv.data();
      if (status) s = hs.data();
    }
    if (hipMemcpyAsync(v, vd, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (s && hipMemcpyAsync(s, pc.words, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    for (size_t r = 0; r < m; r++) {
      if (o.perm) {
        verdicts[first + o.perm[r]] = v[r];
        if (s) status[first + o.perm[r]] = s[r];
      }
      bad += v[r] != BH_OK;
    }
  }
  if (n_bad) *n_bad = bad;
  return BH_OK;
}

// The first proof of a chunk, in the CALLER's order, that Proof::read refused, and its error.  In the caller's order the
// reader's own minimum (hbad) is that proof and its one status word is fetched; through a permutation it is searched in
// the chunk's status words (hwords, in the uploaded order).
int first_unreadable(hipStream_t st, const ProofChunk &pc, const ChunkRows &o, size_t m, unsigned long long hbad,
                     const std::vector<u32> &hwords, size_t *where) {
  if (!o.perm) {
    u32 word = 0;
    if (hipMemcpyAsync(&word, pc.words + hbad, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    *where = (size_t)hbad;
    return proof_status_error(word);
  }
  int err = BH_ERR_HIP;
  *where = ~size_t(0);
  for (size_t r = 0; r < m; r++)
    if (proof_status_error(hwords[r]) != BH_OK && o.perm[r] < *where) {
      *where = o.perm[r];
      err = proof_status_error(hwords[r]);
    }
  return err;
}

// batch::Verifier::verify (groth16/src/verifier/batch.rs:93-192) with the caller's z_j:
//   prod_j e([z_j] A_j, -B_j) * e(-sum z_j C_j, -delta) * e(-Psi, -gamma) * e([acc_Y] alpha, beta) == 1
// (e(X, Y) = e(-X, -Y): the prepared key's -gamma / -delta lines serve both verifiers).  Over a set, with E_j the value
// whose being 1 is proof j's equation under its own key: prod_j E_j^{z_j} == 1 - the product over the keys of the line
// above, under ONE final exponentiation.  Per chunk: one column-sum launch, one multiexp job for sum z_j C_j per key that
// has rows (all issued before the first wait); the tail runs [acc_Y,k] alpha_k, Psi_k per key, and ONE Miller launch
// over the 3 K key pairs.  A key without a proof in the batch takes no part (three identities).
// src: affine records (384 B each), or Proof::write's 192 B per proof, decoded chunk by chunk on the call's stream.  The
// batch is walked ONCE: a chunk is decoded right in front of its Miller loops; the first chunk with a bad proof ends the
// call with the read error of its first bad proof in the caller's order - chunks are taken in stream order, so it is the
// first bad proof of the batch - and as the verdict only exists after the last chunk, a read error anywhere comes before
// BH_ERR_INVALID_PROOF.  The arguments are checked, but for z != 0.
template <class Keys>
int batch_verify(Keys &keys, const void *src, bool compressed, size_t n_proofs, const void *inputs, int scalar_fmt, const void *z,
                 size_t *bad_index) {
  if (!n_proofs) return BH_OK;   // no Miller terms: the reference's empty batch
  for (size_t j = 0; j < n_proofs; j++)
    if (scalar_is_zero_mod_q((const uint8_t *)z + 32 * j)) return BH_ERR_INVALID_ARG;   // batch.rs:117-128: z != 0
  bh_ctx *ctx = keys.ctx();
  CallFrame fr(ctx);
  if (fr.rc) return fr.rc;
  hipStream_t st = fr.st;
  PoolBufs &bufs = fr.bufs;
  const size_t nk = keys.n_keys(), ncol = keys.total_cols();
  const size_t ch = chunk_rows(n_proofs, keys.widest());
  ProofChunk pc;
  const bool have_pc = pc.alloc(bufs, ch, compressed);
  fr_t *zd = bufs.get<fr_t>(ch);
  fr_t *ind = bufs.get<fr_t>(most_scalars(keys, n_proofs, ch));
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(ch);
  Affine<FpOps> *cb = bufs.get<Affine<FpOps>>(ch);
  fr_t *zc = bufs.get<fr_t>(ch);
  line_t *lines = bufs.get<line_t>(ch * MILLER_LINES);
  u32 *pflags = bufs.get<u32>(ch), *qflags = bufs.get<u32>(ch + 1);
  fp12_t *f = bufs.get<fp12_t>(ch + 1);
  fp12_t *facc = bufs.get<fp12_t>(1);
  fr_t *part = bufs.get<fr_t>(ncol * COLSUM_BLOCKS);
  fr_t *acc = bufs.get<fr_t>(ncol);
  Affine<FpOps> *key = bufs.get<Affine<FpOps>>(3 * nk);   // [-Psi_k], [-sum z C of k], [[acc_Y,k] alpha_k]
  Affine<FpOps> *gen = bufs.get<Affine<FpOps>>(1);
  fp12_t *fk = bufs.get<fp12_t>(3 * nk + 1 + 5);          // the key pairs' values, the running product, final exponentiation
  if (!have_pc || !zd || !ind || !pts || !cb || !zc || !lines || !pflags || !qflags || !f || !facc || !part || !acc || !key ||
      !gen || !fk || !keys.alloc_batch(bufs)) {
    fprintf(stderr, "[bellman_hip] batch verification: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  fp12_t one;
  f12_one(one);
  Affine<FpOps> g;
  g1_generator(g);
  if (hipMemcpyAsync(facc, &one, sizeof one, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(gen, &g, sizeof g, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(acc, 0, ncol * sizeof(fr_t), st) != hipSuccess)
    return BH_ERR_HIP;
  std::vector<Affine<FpOps>> sum_c(nk), part_c(nk);   // per key (host, affine): sum z_j C_j over the chunks so far, of one chunk
  memset(sum_c.data(), 0, nk * sizeof(Affine<FpOps>));
  std::vector<unsigned char> active(nk, 0);
  std::vector<bh_bases *> cbases(nk, nullptr);
  std::vector<bh_msm_job *> jobs(nk, nullptr);
  const size_t rec = compressed ? 192 : sizeof(ProofRec);
  std::vector<u32> hflags(ch), hqflags(ch), hwords;   // hwords: a permuted chunk's status words
  unsigned long long hbad = ~0ULL;                    // first proof of the chunk that Proof::read refuses
  u32 bad = 0;
  int rc = BH_OK;
  for (size_t first = 0; first < n_proofs && !rc; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    const ChunkRows o = keys.rows(src, rec, inputs, z, first, m);
    const bool want_words = compressed && o.perm;
    hwords.resize(want_words ? m : 0);
    hbad = ~0ULL;
    if ((rc = keys.upload_layout(st, false))) break;
    if ((rc = pc.upload(st, o.recs, m, true, &hbad))) break;
    if (hipMemcpyAsync(zd, o.z, m * 32, hipMemcpyHostToDevice, st) != hipSuccess ||
        (o.n_in && hipMemcpyAsync(ind, o.inputs, o.n_in * 32, hipMemcpyHostToDevice, st) != hipSuccess)) {
      rc = BH_ERR_HIP;
      break;
    }
    if ((rc = launch_proof_prep(st, pc.pr, zd, scalar_fmt, pts, cb, zc, gen, pflags, m))) break;
    if ((rc = launch_g2_lines(st, &pc.pr->b, sizeof(ProofRec), 1, lines, qflags, m))) break;   // -B_j
    if ((rc = keys.colsum(st, zd, ind, scalar_fmt, m, part, acc))) break;
    // sum z_j C_j of every key's run on the multiexp path, ordered after the prep kernel: all issued before the first wait
    for (size_t k = 0; k < nk && !rc; k++) {
      const KeySeg s = keys.run(k, m);
      if (!s.count) continue;
      active[k] = 1;
      if ((rc = bh_bases_wrap_dev(ctx, BH_G1, cb + s.first, s.count, &cbases[k]))) break;
      rc = bh_msm_async_dev_after(ctx, cbases[k], 0, zc + s.first, s.count, scalar_fmt, nullptr, 0, nullptr, (void *)st, &jobs[k]);
    }
    if (!rc) rc = launch_miller(st, pts, lines, qflags, f, m);
    if (!rc && hipMemcpyAsync(f + m, facc, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
    if (!rc) rc = launch_fold(st, f, m + 1);
    if (!rc && hipMemcpyAsync(facc, f, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
    if (!rc && (hipMemcpyAsync(hflags.data(), pflags, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(hqflags.data(), qflags, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                (want_words && hipMemcpyAsync(hwords.data(), pc.words, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess)))
      rc = BH_ERR_HIP;
    for (size_t k = 0; k < nk; k++)
      if (jobs[k]) {
        const int mrc = bh_msm_wait(jobs[k], &part_c[k]);
        if (!rc) rc = mrc;
      }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
    for (size_t k = 0; k < nk; k++) {
      if (cbases[k]) bh_bases_release(ctx, cbases[k]);
      cbases[k] = nullptr;
      if (jobs[k] && !rc) bh_point_add(BH_G1, &sum_c[k], &sum_c[k], &part_c[k], 1);
      jobs[k] = nullptr;
    }
    if (rc) break;
    if (hbad != ~0ULL) {   // Proof::read failed in this chunk (its points went on as identities; the result is dropped)
      size_t where = 0;
      const int err = first_unreadable(st, pc, o, m, hbad, hwords, &where);
      if (err != BH_ERR_HIP && bad_index) *bad_index = first + where;
      return err;
    }
    for (size_t j = 0; j < m; j++) bad |= hflags[j] | (hqflags[j] & PF_OFF_CURVE);
  }
  if (rc) return rc;
  if (bad & PF_OFF_CURVE) return BH_ERR_INVALID_POINT;
  // [acc_Y,k] alpha_k (acc_Y = acc_Gamma_0), then Psi_k = sum acc_Gamma_{k,i} ic_{k,i} with the scalars of identity ic_i
  // zeroed (they take no part; the zeroing is ordered after the read of acc_Y,k)
  if ((rc = keys.mul_alpha(st, key + 2 * nk, acc))) return rc;
  for (size_t k = 0; k < nk; k++) {
    const bh_pvk *pvk = keys.key(k);
    for (size_t i = 0; i < pvk->n_ic; i++)
      if (pvk->ic_identity[i] && hipMemsetAsync(acc + keys.col_off(k) + i, 0, sizeof(fr_t), st) != hipSuccess) return BH_ERR_HIP;
  }
  for (size_t k = 0; k < nk && !rc; k++)
    if (active[k])
      rc = bh_msm_async_dev_after(ctx, keys.key(k)->ic, 0, acc + keys.col_off(k), keys.key(k)->n_ic, BH_SCALARS_MONT, nullptr, 0,
                                  nullptr, (void *)st, &jobs[k]);
  std::vector<Affine<FpOps>> k2(2 * nk);
  memset(k2.data(), 0, 2 * nk * sizeof(Affine<FpOps>));
  for (size_t k = 0; k < nk; k++) {
    if (!jobs[k]) continue;
    Affine<FpOps> psi;
    const int mrc = bh_msm_wait(jobs[k], &psi);
    if (!rc) rc = mrc;
    neg_g1_host(k2[k], psi);
    neg_g1_host(k2[nk + k], sum_c[k]);
  }
  if (rc) return rc;
  if (hipMemcpyAsync(key, k2.data(), 2 * nk * sizeof(Affine<FpOps>), hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
  if ((rc = keys.miller_pairs(st, key, fk))) return rc;
  bool ok = false;
  if ((rc = finish_product(st, fk, 3 * nk, facc, qflags, &ok))) return rc;
  return ok ? BH_OK : BH_ERR_INVALID_PROOF;
}
}  // namespace

extern "C" {

int bh_groth16_batch_verify(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                            int scalar_fmt, const void *z) {
  if (const int rc = one_key_check_args(pvk, proofs, z, n_proofs, inputs, n_inputs, scalar_fmt)) return rc;
  OneKey keys{pvk};
  return batch_verify(keys, proofs, false, n_proofs, inputs, scalar_fmt, z, nullptr);
}

// Proof::read of every proof (groth16/src/lib.rs:47-99), then batch::Verifier::verify, the decoded proofs never leaving
// the device
int bh_groth16_batch_verify_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                       size_t n_inputs, int scalar_fmt, const void *z, size_t *bad_index) {
  if (const int rc = one_key_check_args(pvk, bytes, z, n_proofs, inputs, n_inputs, scalar_fmt)) return rc;
  OneKey keys{pvk};
  return batch_verify(keys, bytes, true, n_proofs, inputs, scalar_fmt, z, bad_index);
}

// Proof::read over n concatenated 192-byte proofs: chunks of at most BATCH_CHUNK proofs on a stream of the call's own
int bh_proofs_read(bh_ctx *ctx, const void *bytes, size_t n_proofs, void *out_proofs_affine, uint32_t *status,
                   size_t *bad_index) {
  if (!ctx || (n_proofs && (!bytes || !out_proofs_affine))) return BH_ERR_INVALID_ARG;
  if (!n_proofs) return BH_OK;
  CallFrame fr(ctx);
  if (fr.rc) return fr.rc;
  hipStream_t st = fr.st;
  const size_t ch = chunk_rows(n_proofs, 0);
  ProofChunk pc;
  if (!pc.alloc(fr.bufs, ch, true)) return BH_ERR_HIP;
  std::vector<u32> words(ch);
  int result = BH_OK;
  for (size_t first = 0; first < n_proofs; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    unsigned long long hbad = ~0ULL;
    // (first_bad comes down behind the records and the status words, with the one synchronisation)
    const int rc = pc.upload(st, (const unsigned char *)bytes + first * 192, m, true, nullptr);
    if (rc) return rc;
    if (hipMemcpyAsync((ProofRec *)out_proofs_affine + first, pc.pr, m * sizeof(ProofRec), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(words.data(), pc.words, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&hbad, pc.first_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    if (status) memcpy(status + first, words.data(), m * 4);
    if (hbad != ~0ULL && result == BH_OK) {
      result = proof_status_error(words[hbad]);
      if (bad_index) *bad_index = first + (size_t)hbad;
    }
  }
  return result;
}

// batch::Item::verify_single (batch.rs:55-66) = verify_proof (verifier.rs:23-58) of every proof, verdict by verdict
int bh_groth16_verify_each(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                           int scalar_fmt, int32_t *verdicts, size_t *n_bad) {
  if (pvk && n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;   // verifier.rs:27-29, before anything else
  if (const int rc = one_key_check_args(pvk, proofs, verdicts, n_proofs, inputs, n_inputs, scalar_fmt)) return rc;
  OneKey keys{pvk};
  return verify_each(keys, proofs, false, n_proofs, inputs, scalar_fmt, verdicts, nullptr, n_bad);
}

// the same from the bytes of Proof::write: Proof::read (groth16/src/lib.rs:47-99) of proof j, then verify_proof
// (verifier.rs:23-58) / Item::verify_single (batch.rs:55-66); the decoded proofs stay on the device
int bh_groth16_verify_each_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                      size_t n_inputs, int scalar_fmt, int32_t *verdicts, uint32_t *status, size_t *n_bad) {
  if (pvk && n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;
  if (const int rc = one_key_check_args(pvk, bytes, verdicts, n_proofs, inputs, n_inputs, scalar_fmt)) return rc;
  OneKey keys{pvk};
  return verify_each(keys, bytes, true, n_proofs, inputs, scalar_fmt, verdicts, status, n_bad);
}

int bh_groth16_pvk_set_create(const bh_pvk *const *pvks, size_t n_keys, bh_pvk_set **out) {
  if (!pvks || !out || !n_keys || n_keys > BH_PVK_SET_MAX_KEYS) return BH_ERR_INVALID_ARG;
  for (size_t k = 0; k < n_keys; k++)
    if (!pvks[k] || pvks[k]->ctx != pvks[0]->ctx) return BH_ERR_INVALID_ARG;
  std::unique_ptr<bh_pvk_set> s(new bh_pvk_set);
  s->ctx = pvks[0]->ctx;
  Context &c = s->ctx->c;
  CallFrame fr(s->ctx);
  if (fr.rc) return fr.rc;
  s->keys.assign(pvks, pvks + n_keys);
  s->host.resize(n_keys);
  for (size_t k = 0; k < n_keys; k++) {
    const bh_pvk *p = pvks[k];
    KeyDesc &d = s->host[k];
    memset(&d, 0, sizeof d);
    d.lines = p->lines;
    d.qflags = p->qflags;
    d.alpha = p->alpha_dev;
    d.w = 8;
    d.n_inputs = (u32)(p->n_ic - 1);
    d.col_off = (u32)s->total_cols;
    s->total_cols += p->n_ic;
    s->max_in = std::max(s->max_in, p->n_ic - 1);
  }
  s->dev = (KeyDesc *)c.pool.acquire(2 * n_keys * sizeof(KeyDesc));
  if (!s->dev) return BH_ERR_HIP;
  if (hipMemcpyAsync(s->dev, s->host.data(), n_keys * sizeof(KeyDesc), hipMemcpyHostToDevice, fr.st) != hipSuccess ||
      hipStreamSynchronize(fr.st) != hipSuccess) {
    c.pool.release(s->dev);
    return BH_ERR_HIP;
  }
  *out = s.release();
  return BH_OK;
}

size_t bh_groth16_pvk_set_len(const bh_pvk_set *set) { return set ? set->keys.size() : 0; }

void bh_groth16_pvk_set_release(bh_pvk_set *set) {
  if (!set) return;
  Context &c = set->ctx->c;
  (void)hipSetDevice(c.device);
  c.pool.release(set->dev);
  delete set;
}

int bh_groth16_verify_each_keys(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, size_t n_proofs,
                                const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts, size_t *n_bad) {
  SetKeys keys;
  if (const int rc = keys.init(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt)) return rc;
  if (n_proofs && (!proofs || !verdicts)) return BH_ERR_INVALID_ARG;
  return verify_each(keys, proofs, false, n_proofs, inputs, scalar_fmt, verdicts, nullptr, n_bad);
}

int bh_groth16_verify_each_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                           const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts,
                                           uint32_t *status, size_t *n_bad) {
  SetKeys keys;
  if (const int rc = keys.init(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt)) return rc;
  if (n_proofs && (!bytes || !verdicts)) return BH_ERR_INVALID_ARG;
  return verify_each(keys, bytes, true, n_proofs, inputs, scalar_fmt, verdicts, status, n_bad);
}

int bh_groth16_batch_verify_keys(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, size_t n_proofs,
                                 const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z) {
  SetKeys keys;
  if (const int rc = keys.init(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt)) return rc;
  if (n_proofs && (!proofs || !z)) return BH_ERR_INVALID_ARG;
  return batch_verify(keys, proofs, false, n_proofs, inputs, scalar_fmt, z, nullptr);
}

int bh_groth16_batch_verify_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                            const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z,
                                            size_t *bad_index) {
  SetKeys keys;
  if (const int rc = keys.init(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt)) return rc;
  if (n_proofs && (!bytes || !z)) return BH_ERR_INVALID_ARG;
  return batch_verify(keys, bytes, true, n_proofs, inputs, scalar_fmt, z, bad_index);
}

}  // extern "C"
