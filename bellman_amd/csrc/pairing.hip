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

// the pairing check itself: n_chunks of proofs were folded into facc; now the three key pairs, the product, the
// final exponentiation.  key_p: the three G1 points (device) paired with -gamma, -delta, beta.
// The pairing check: the three key pairs (key_p: the G1 points paired with -gamma, -delta, beta) - after n_own pairs of
// the caller's (P at key_p - n_own, lines own_lines) in the same launch - times facc (the proofs' product so far, may be
// NULL), then the final exponentiation.
int finish_check(hipStream_t st, const bh_pvk *pvk, PoolBufs &bufs, const Affine<FpOps> *key_p_dev, size_t n_own,
                 const line_t *own_lines, const u32 *own_flags, const fp12_t *facc, u32 *is_one_dev, bool *is_one) {
  fp12_t *fk = bufs.get<fp12_t>(n_own + 4 + 5);   // the pairs' values, the running product, final exponentiation workspace
  if (!fk) return BH_ERR_HIP;
  fp12_t *fe = fk + n_own + 4;
  int rc = n_own ? launch_miller(st, key_p_dev - n_own, own_lines, own_flags, fk, n_own, pvk->lines, pvk->qflags, 3)
                 : launch_miller(st, key_p_dev, pvk->lines, pvk->qflags, fk, 3);
  if (rc) return rc;
  size_t m = n_own + 3;
  if (facc) {
    if (hipMemcpyAsync(fk + m, facc, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return BH_ERR_HIP;
    m++;
  }
  if ((rc = launch_fold(st, fk, m))) return rc;
  if ((rc = launch_final_exp(st, fk, 1, fe, is_one_dev, fe + 1))) return rc;
  u32 h = 0;
  if (hipMemcpyAsync(&h, is_one_dev, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return BH_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return BH_ERR_HIP;
  *is_one = h == 1;
  return BH_OK;
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
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
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
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  ProofRec *pr = bufs.get<ProofRec>(1);
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(4);   // [A, acc, C, -alpha]
  line_t *lines = bufs.get<line_t>(MILLER_LINES);
  u32 *flags = bufs.get<u32>(4);
  Affine<FpOps> acc;
  Affine<FpOps> key[3];   // source of an asynchronous copy: lives until finish_check has synchronised
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) sh.st = nullptr;
  if (!pr || !pts || !lines || !flags || !sh.st) {
    bh_msm_wait(job, &acc);
    return BH_ERR_HIP;
  }
  hipStream_t st = sh.st;
  const ProofRec *hp = (const ProofRec *)proof;
  if (hipMemcpyAsync(pr, proof, sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
  if (!rc) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, dim3(1), dim3(64), 0, st, pr, (const fr_t *)nullptr, 0, pts, (Affine<FpOps> *)nullptr,
                       (fr_t *)nullptr, (const Affine<FpOps> *)nullptr, flags, 1u);
    if (hipGetLastError() != hipSuccess) rc = BH_ERR_HIP;
  }
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
  if (!rc) rc = finish_check(st, pvk, bufs, pts + 1, 1, lines, flags + 1, nullptr, flags + 3, &one);
  u32 hf[2] = {0, 0};
  if (!rc && (hipMemcpyAsync(hf, flags, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
    rc = BH_ERR_HIP;
  if (rc) return rc;
  if ((hf[0] | hf[1]) & PF_OFF_CURVE) return BH_ERR_INVALID_POINT;
  return one ? BH_OK : BH_ERR_INVALID_PROOF;
}

}  // extern "C"

// batch::Verifier::verify (groth16/src/verifier/batch.rs:93-192) with the caller's z_j:
//   prod_j e([z_j] A_j, -B_j) * e(-sum z_j C_j, -delta) * e(-Psi, -gamma) * e([acc_Y] alpha, beta) == 1
// (e(X, Y) = e(-X, -Y): the prepared key's -gamma / -delta lines serve both verifiers).
// `proofs`: affine records (384 B each), or NULL with `bytes`: Proof::write's 192 B per proof, decoded chunk by chunk on
// the verifier's stream (Proof::read: every point checked, the identity refused).  The batch is walked ONCE: a chunk is
// decoded right in front of its Miller loops; the first chunk with a bad proof ends the call with that proof's read
// error - chunks are taken in stream order, so it is the first bad proof of the batch - and as the verdict only exists
// after the last chunk, a read error anywhere comes before BH_ERR_INVALID_PROOF.
static int batch_verify_impl(const bh_pvk *pvk, const void *proofs, const void *bytes, size_t n_proofs, const void *inputs,
                             size_t n_inputs, int scalar_fmt, const void *z, size_t *bad_index) {
  if (!pvk || (n_proofs && ((!proofs && !bytes) || !z)) || (n_proofs && n_inputs && !inputs) ||
      (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT))
    return BH_ERR_INVALID_ARG;
  if (n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;   // batch.rs:101-107
  if (!n_proofs) return BH_OK;                                           // no Miller terms: the reference's empty batch
  for (size_t j = 0; j < n_proofs; j++)
    if (scalar_is_zero_mod_q((const uint8_t *)z + 32 * j)) return BH_ERR_INVALID_ARG;   // batch.rs:117-128: z != 0
  bh_ctx *ctx = pvk->ctx;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) return BH_ERR_HIP;
  hipStream_t st = sh.st;
  // chunk: at most BATCH_CHUNK proofs, and at most INPUTS_CHUNK_BYTES of public inputs
  const size_t by_inputs = std::max<size_t>(1, INPUTS_CHUNK_BYTES / (32 * std::max<size_t>(n_inputs, 1)));
  const size_t ch = std::min(std::min(n_proofs, BATCH_CHUNK), by_inputs);
  const size_t ncol = pvk->n_ic;
  ProofRec *pr = bufs.get<ProofRec>(ch);
  fr_t *zd = bufs.get<fr_t>(ch);
  fr_t *ind = bufs.get<fr_t>(ch * (n_inputs ? n_inputs : 1));
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(ch);
  Affine<FpOps> *cb = bufs.get<Affine<FpOps>>(ch);
  fr_t *zc = bufs.get<fr_t>(ch);
  line_t *lines = bufs.get<line_t>(ch * MILLER_LINES);
  u32 *pflags = bufs.get<u32>(ch), *qflags = bufs.get<u32>(ch + 1);
  fp12_t *f = bufs.get<fp12_t>(ch + 1);
  fp12_t *facc = bufs.get<fp12_t>(1);
  fr_t *part = bufs.get<fr_t>(ncol * COLSUM_BLOCKS);
  fr_t *acc = bufs.get<fr_t>(ncol);
  Affine<FpOps> *key = bufs.get<Affine<FpOps>>(3);
  Affine<FpOps> *gen = bufs.get<Affine<FpOps>>(1);
  unsigned char *cbytes = bytes ? bufs.get<unsigned char>(ch * 192) : nullptr;   // the chunk as written, its per-point and
  u32 *pst = bytes ? bufs.get<u32>(4 * ch) : nullptr;                            // per-proof status words, the first bad proof
  unsigned long long *first_bad = bytes ? bufs.get<unsigned long long>(1) : nullptr;
  if (bytes && (!cbytes || !pst || !first_bad)) return BH_ERR_HIP;
  if (!pr || !zd || !ind || !pts || !cb || !zc || !lines || !pflags || !qflags || !f || !facc || !part || !acc || !key || !gen) {
    fprintf(stderr, "[bellman_hip] batch verification: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  fp12_t one;
  f12_one(one);
  Affine<FpOps> g;
  g1_generator(g);
  int rc = BH_OK;
  if (hipMemcpyAsync(facc, &one, sizeof one, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(gen, &g, sizeof g, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(acc, 0, ncol * sizeof(fr_t), st) != hipSuccess)
    return BH_ERR_HIP;
  Affine<FpOps> sum_c;   // sum z_j C_j over the chunks so far (host, affine)
  memset(&sum_c, 0, sizeof sum_c);
  u32 bad = 0;
  std::vector<u32> hflags(ch), hqflags(ch);
  unsigned long long hbad = ~0ULL;   // first proof of the chunk that Proof::read refuses
  for (size_t first = 0; first < n_proofs && !rc; first += ch) {
    const size_t m = n_proofs - first < ch ? n_proofs - first : ch;
    hbad = ~0ULL;
    if (bytes) {
      if (hipMemcpyAsync(cbytes, (const unsigned char *)bytes + first * 192, m * 192, hipMemcpyHostToDevice, st) != hipSuccess ||
          hipMemsetAsync(first_bad, 0xff, 8, st) != hipSuccess) {
        rc = BH_ERR_HIP;
        break;
      }
      if ((rc = proofs_read_dev(cbytes, pr, m, pst, pst + 3 * ch, first_bad, st))) break;
      if (hipMemcpyAsync(&hbad, first_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = BH_ERR_HIP; break; }
    } else if (hipMemcpyAsync(pr, (const ProofRec *)proofs + first, m * sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = BH_ERR_HIP;
      break;
    }
    if (hipMemcpyAsync(zd, (const fr_t *)z + first, m * 32, hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_inputs && hipMemcpyAsync(ind, (const fr_t *)inputs + first * n_inputs, m * n_inputs * 32, hipMemcpyHostToDevice, st) !=
                         hipSuccess)) {
      rc = BH_ERR_HIP;
      break;
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, pr, zd, scalar_fmt, pts, cb, zc, gen, pflags,
                       (u32)m);
    if (hipGetLastError() != hipSuccess) { rc = BH_ERR_HIP; break; }
    if ((rc = launch_g2_lines(st, &pr->b, sizeof(ProofRec), 1, lines, qflags, m))) break;   // -B_j
    if ((rc = launch_colsum(st, zd, ind, n_inputs, scalar_fmt, m, part, acc))) break;
    // sum z_j C_j of this chunk on the multiexp path, ordered after the prep kernel
    bh_bases *cbases = nullptr;
    bh_msm_job *job = nullptr;
    if ((rc = bh_bases_wrap_dev(ctx, BH_G1, cb, m, &cbases))) break;
    rc = bh_msm_async_dev_after(ctx, cbases, 0, zc, m, scalar_fmt, nullptr, 0, nullptr, (void *)st, &job);
    if (!rc) rc = launch_miller(st, pts, lines, qflags, f, m);
    if (!rc && hipMemcpyAsync(f + m, facc, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
    if (!rc) rc = launch_fold(st, f, m + 1);
    if (!rc && hipMemcpyAsync(facc, f, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BH_ERR_HIP;
    if (!rc && (hipMemcpyAsync(hflags.data(), pflags, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(hqflags.data(), qflags, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess))
      rc = BH_ERR_HIP;
    Affine<FpOps> part_c;
    if (job) {
      const int mrc = bh_msm_wait(job, &part_c);
      if (!rc) rc = mrc;
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = BH_ERR_HIP;
    bh_bases_release(ctx, cbases);
    if (rc) break;
    if (hbad != ~0ULL) {   // Proof::read failed in this chunk (its points went on as identities; the result is dropped)
      u32 word = 0;
      if (hipMemcpyAsync(&word, pst + 3 * ch + hbad, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return BH_ERR_HIP;
      if (bad_index) *bad_index = first + (size_t)hbad;
      return proof_status_error(word);
    }
    bh_point_add(BH_G1, &sum_c, &sum_c, &part_c, 1);
    for (size_t j = 0; j < m; j++) bad |= hflags[j] | (hqflags[j] & PF_OFF_CURVE);
  }
  if (rc) return rc;
  if (bad & PF_OFF_CURVE) return BH_ERR_INVALID_POINT;
  // [acc_Y] alpha (acc_Y = acc_Gamma_0), then Psi = sum acc_Gamma_i ic_i with the scalars of identity ic_i zeroed (they take
  // no part; the zeroing is ordered after the read of acc_Y)
  (void)hipGetLastError();
  hipLaunchKernelGGL(g1_mul_one_kernel, dim3(1), dim3(64), 0, st, key + 2, pvk->alpha_dev, (const fr_t *)acc);
  if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
  for (size_t i = 0; i < ncol; i++)
    if (pvk->ic_identity[i] && hipMemsetAsync(acc + i, 0, sizeof(fr_t), st) != hipSuccess) return BH_ERR_HIP;
  bh_msm_job *job = nullptr;
  if ((rc = bh_msm_async_dev_after(ctx, pvk->ic, 0, acc, ncol, BH_SCALARS_MONT, nullptr, 0, nullptr, (void *)st, &job))) return rc;
  Affine<FpOps> psi;
  const int mrc = bh_msm_wait(job, &psi);
  if (!rc) rc = mrc;
  if (rc) return rc;
  Affine<FpOps> k2[2];
  neg_g1_host(k2[0], psi);
  neg_g1_host(k2[1], sum_c);
  if (hipMemcpyAsync(key, k2, sizeof k2, hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
  bool ok = false;
  if ((rc = finish_check(st, pvk, bufs, key, 0, nullptr, nullptr, facc, qflags, &ok))) return rc;
  return ok ? BH_OK : BH_ERR_INVALID_PROOF;
}

extern "C" {

int bh_groth16_batch_verify(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                            int scalar_fmt, const void *z) {
  if (n_proofs && !proofs) return BH_ERR_INVALID_ARG;
  return batch_verify_impl(pvk, proofs, nullptr, n_proofs, inputs, n_inputs, scalar_fmt, z, nullptr);
}

// Proof::read of every proof (groth16/src/lib.rs:47-99), then batch::Verifier::verify, the decoded proofs never leaving
// the device
int bh_groth16_batch_verify_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                       size_t n_inputs, int scalar_fmt, const void *z, size_t *bad_index) {
  if (n_proofs && !bytes) return BH_ERR_INVALID_ARG;
  return batch_verify_impl(pvk, nullptr, bytes, n_proofs, inputs, n_inputs, scalar_fmt, z, bad_index);
}

// Proof::read over n concatenated 192-byte proofs: chunks of at most BATCH_CHUNK proofs on a stream of the call's own
int bh_proofs_read(bh_ctx *ctx, const void *bytes, size_t n_proofs, void *out_proofs_affine, uint32_t *status,
                   size_t *bad_index) {
  if (!ctx || (n_proofs && (!bytes || !out_proofs_affine))) return BH_ERR_INVALID_ARG;
  if (!n_proofs) return BH_OK;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) return BH_ERR_HIP;
  hipStream_t st = sh.st;
  const size_t ch = std::min(n_proofs, BATCH_CHUNK);
  unsigned char *cbytes = bufs.get<unsigned char>(ch * 192);
  ProofRec *pr = bufs.get<ProofRec>(ch);
  u32 *pst = bufs.get<u32>(4 * ch);
  unsigned long long *first_bad = bufs.get<unsigned long long>(1);
  if (!cbytes || !pr || !pst || !first_bad) return BH_ERR_HIP;
  std::vector<u32> words(ch);
  int result = BH_OK;
  for (size_t first = 0; first < n_proofs; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    unsigned long long hbad = ~0ULL;
    if (hipMemcpyAsync(cbytes, (const unsigned char *)bytes + first * 192, m * 192, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(first_bad, 0xff, 8, st) != hipSuccess)
      return BH_ERR_HIP;
    const int rc = proofs_read_dev(cbytes, pr, m, pst, pst + 3 * ch, first_bad, st);
    if (rc) return rc;
    if (hipMemcpyAsync((ProofRec *)out_proofs_affine + first, pr, m * sizeof(ProofRec), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(words.data(), pst + 3 * ch, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&hbad, first_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    if (status) memcpy(status + first, words.data(), m * 4);
    if (hbad != ~0ULL && result == BH_OK) {
      result = proof_status_error(words[hbad]);
      if (bad_index) *bad_index = first + (size_t)hbad;
    }
  }
  return result;
}

}  // extern "C"

// ---- per-proof verdicts: Item::verify_single for every proof of a batch (groth16/src/verifier/batch.rs:55-66, which is
// verify_proof, groth16/src/verifier.rs:23-58) in one call --------------------------------------------------------------
// Every proof takes one lane through: proof_prep_kernel / g2_lines_kernel (curve flags, B_j's lines), ic_accumulate_kernel
// (acc_j from the key's window table), miller3_kernel (three pairs, shared squarings), f12_mul_const_kernel (the key's
// f(-alpha, beta)), the n-wide final exponentiation chain and verdict_kernel.  No multiexp job, no host loop over proofs;
// one download and one synchronisation per chunk.
namespace {
// the key's share, once per key: the largest window of 8, 4, 2, 1 bits whose table fits the context's table budget
void build_each(const bh_pvk *pvk) {
  bh_pvk::Each &e = pvk->each;
  bh_ctx *ctx = pvk->ctx;
  Context &c = ctx->c;
  const size_t n_in = pvk->n_ic - 1;
  e.rc = BH_ERR_HIP;
  if (hipSetDevice(c.device) != hipSuccess) return;
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
  Affine<FpOps> *icd = (Affine<FpOps> *)c.pool.acquire(pvk->n_ic * sizeof(Affine<FpOps>));
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) sh.st = nullptr;
  if (e.ic0 && icd && sh.st) {
    hipStream_t st = sh.st;
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
  c.pool.release(icd);
}

int verify_each_impl(const bh_pvk *pvk, const void *proofs, const void *bytes, size_t n_proofs, const void *inputs,
                     size_t n_inputs, int scalar_fmt, int32_t *verdicts, uint32_t *status, size_t *n_bad) {
  if (!pvk || (n_proofs && ((!proofs && !bytes) || !verdicts)) || (n_proofs && n_inputs && !inputs) ||
      (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT))
    return BH_ERR_INVALID_ARG;
  if (n_bad) *n_bad = 0;
  if (!n_proofs) return BH_OK;
  bh_ctx *ctx = pvk->ctx;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  std::call_once(pvk->each.once, build_each, pvk);
  const bh_pvk::Each &e = pvk->each;
  if (e.rc) return e.rc;
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) return BH_ERR_HIP;
  hipStream_t st = sh.st;
  const bool separate = !env().verify_each_shared;   // three one-pair loops: the faster form at 2^14 proofs, see miller3_kernel
  const size_t by_inputs = std::max<size_t>(1, INPUTS_CHUNK_BYTES / (32 * std::max<size_t>(n_inputs, 1)));
  const size_t ch = std::min(std::min(n_proofs, BATCH_CHUNK), by_inputs);
  ProofRec *pr = bufs.get<ProofRec>(ch);
  fr_t *ind = bufs.get<fr_t>(ch * (n_inputs ? n_inputs : 1));
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(2 * ch);   // A_j, then acc_j
  line_t *lines = bufs.get<line_t>(ch * MILLER_LINES);
  u32 *words = bufs.get<u32>(5 * ch);                     // curve flags of A/C, of B, is_one, verdicts, status words
  fp12_t *f = bufs.get<fp12_t>((separate ? 3 : 1) * ch);
  fp12_t *ws = bufs.get<fp12_t>(4 * ch);                  // final exponentiation workspace
  unsigned char *cbytes = bytes ? bufs.get<unsigned char>(ch * 192) : nullptr;
  u32 *pst = bytes ? bufs.get<u32>(3 * ch) : nullptr;
  unsigned long long *first_bad = bytes ? bufs.get<unsigned long long>(1) : nullptr;   // (the reader's; not used here)
  if (!pr || !ind || !pts || !lines || !words || !f || !ws || (bytes && (!cbytes || !pst || !first_bad))) {
    fprintf(stderr, "[bellman_hip] verify_each: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  u32 *pflags = words, *qflags = words + ch, *is_one = words + 2 * ch, *wst = bytes ? words + 4 * ch : nullptr;
  int *vd = (int *)(words + 3 * ch);
  Affine<FpOps> *accp = pts + ch;
  size_t bad = 0;
  for (size_t first = 0; first < n_proofs; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    if (bytes) {
      if (hipMemcpyAsync(cbytes, (const unsigned char *)bytes + first * 192, m * 192, hipMemcpyHostToDevice, st) != hipSuccess)
        return BH_ERR_HIP;
      const int rc = proofs_read_dev(cbytes, pr, m, pst, wst, first_bad, st);
      if (rc) return rc;
    } else if (hipMemcpyAsync(pr, (const ProofRec *)proofs + first, m * sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) {
      return BH_ERR_HIP;
    }
    if (n_inputs && hipMemcpyAsync(ind, (const fr_t *)inputs + first * n_inputs, m * n_inputs * 32, hipMemcpyHostToDevice, st) != hipSuccess)
      return BH_ERR_HIP;
    const dim3 g(blocks_of(m, 64)), blk(64);
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, g, blk, 0, st, pr, (const fr_t *)nullptr, 0, pts, (Affine<FpOps> *)nullptr, (fr_t *)nullptr,
                       (const Affine<FpOps> *)nullptr, pflags, (u32)m);
    hipLaunchKernelGGL(ic_accumulate_kernel, g, blk, 0, st, ind, (u32)n_inputs, scalar_fmt, e.table, e.w ? e.w : 8u, e.ic0, accp,
                       (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    int rc = launch_g2_lines(st, &pr->b, sizeof(ProofRec), 0, lines, qflags, m);
    if (rc) return rc;
    hipLaunchKernelGGL(miller3_kernel, dim3(g.x, separate ? 3 : 1), blk, 0, st, pts, accp, pr, lines, qflags, pvk->lines, pvk->qflags,
                       7u, f, (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    if ((rc = launch_fold3_const(st, f, e.f_ab, m, separate))) return rc;
    if ((rc = launch_final_exp(st, f, m, f, is_one, ws))) return rc;
    hipLaunchKernelGGL(verdict_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, st, wst, pflags, qflags, is_one, vd, (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    if (hipMemcpyAsync(verdicts + first, vd, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (status && hipMemcpyAsync(status + first, wst, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    for (size_t j = 0; j < m; j++) bad += verdicts[first + j] != BH_OK;
  }
  if (n_bad) *n_bad = bad;
  return BH_OK;
}
}  // namespace

extern "C" {

// batch::Item::verify_single (batch.rs:55-66) = verify_proof (verifier.rs:23-58) of every proof, verdict by verdict
int bh_groth16_verify_each(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                           int scalar_fmt, int32_t *verdicts, size_t *n_bad) {
  if (pvk && n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;   // verifier.rs:27-29, before anything else
  if (n_proofs && !proofs) return BH_ERR_INVALID_ARG;
  return verify_each_impl(pvk, proofs, nullptr, n_proofs, inputs, n_inputs, scalar_fmt, verdicts, nullptr, n_bad);
}

// the same from the bytes of Proof::write: Proof::read (groth16/src/lib.rs:47-99) of proof j, then verify_proof
// (verifier.rs:23-58) / Item::verify_single (batch.rs:55-66); the decoded proofs stay on the device
int bh_groth16_verify_each_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                      size_t n_inputs, int scalar_fmt, int32_t *verdicts, uint32_t *status, size_t *n_bad) {
  if (pvk && n_inputs + 1 != pvk->n_ic) return BH_ERR_INVALID_VERIFYING_KEY;
  if (n_proofs && !bytes) return BH_ERR_INVALID_ARG;
  return verify_each_impl(pvk, nullptr, bytes, n_proofs, inputs, n_inputs, scalar_fmt, verdicts, status, n_bad);
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
void set_build_each(const bh_pvk_set *set) {
  Context &c = set->ctx->c;
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
  if (hipSetDevice(c.device) != hipSuccess) return;
  StreamHold sh(set->ctx);
  if (bh_stream_create(set->ctx, (void **)&sh.st) != BH_OK) {
    sh.st = nullptr;
    return;
  }
  if (hipMemcpyAsync(set->dev + d.size(), d.data(), d.size() * sizeof(KeyDesc), hipMemcpyHostToDevice, sh.st) != hipSuccess ||
      hipStreamSynchronize(sh.st) != hipSuccess)
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

// the call-level checks both forms share; offs[j]: the first scalar of proof j in `inputs` (n_proofs + 1 values)
int keys_check_args(const bh_pvk_set *set, const uint32_t *key_of, size_t n_proofs, const void *inputs, size_t n_inputs_total,
                    int scalar_fmt, std::vector<size_t> &offs) {
  if (!set || (n_proofs && !key_of) || (scalar_fmt != BH_SCALARS_CANONICAL && scalar_fmt != BH_SCALARS_MONT)) return BH_ERR_INVALID_ARG;
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
// chunk: at most BATCH_CHUNK proofs, and at most INPUTS_CHUNK_BYTES of public inputs if every proof had the widest key
size_t keys_chunk(const bh_pvk_set *set, size_t n_proofs) {
  const size_t by_inputs = std::max<size_t>(1, INPUTS_CHUNK_BYTES / (32 * std::max<size_t>(set->max_in, 1)));
  return std::min(std::min(n_proofs, BATCH_CHUNK), by_inputs);
}
// the chunk's records (rec bytes each) and inputs in grouped order
void keys_gather(const Grouping &g, const bh_pvk_set *set, const uint32_t *key_of, const unsigned char *recs, size_t rec,
                 const unsigned char *inputs, const size_t *offs, std::vector<unsigned char> &hrec, std::vector<unsigned char> &hin) {
  const size_t m = g.perm.size();
  hrec.resize(m * rec);
  hin.resize(std::max<size_t>(g.n_in, 1) * 32);
  size_t in = 0;
  for (size_t r = 0; r < m; r++) {
    const size_t j = g.perm[r];
    memcpy(&hrec[r * rec], recs + j * rec, rec);
    const size_t cnt = set->host[key_of[j]].n_inputs;
    if (cnt) memcpy(&hin[in * 32], inputs + offs[j] * 32, cnt * 32);
    in += cnt;
  }
}

int verify_each_keys_impl(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, const void *bytes, size_t n_proofs,
                          const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts, uint32_t *status,
                          size_t *n_bad) {
  std::vector<size_t> offs;
  int rc = keys_check_args(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt, offs);
  if (rc) return rc;
  if (n_proofs && ((!proofs && !bytes) || !verdicts)) return BH_ERR_INVALID_ARG;
  if (n_bad) *n_bad = 0;
  if (!n_proofs) return BH_OK;
  bh_ctx *ctx = set->ctx;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  std::call_once(set->each_once, set_build_each, set);
  if (set->each_rc) return set->each_rc;
  const size_t nk = set->keys.size();
  const KeyDesc *kd = set->dev + nk;
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) return BH_ERR_HIP;
  hipStream_t st = sh.st;
  const bool separate = !env().verify_each_shared;
  const size_t ch = keys_chunk(set, n_proofs);
  size_t in_max = 1;   // the most scalars any chunk holds
  for (size_t first = 0; first < n_proofs; first += ch)
    in_max = std::max(in_max, offs[std::min(first + ch, n_proofs)] - offs[first]);
  const size_t max_blocks = ch / 64 + nk + 1;
  ProofRec *pr = bufs.get<ProofRec>(ch);
  fr_t *ind = bufs.get<fr_t>(in_max);
  Affine<FpOps> *pts = bufs.get<Affine<FpOps>>(2 * ch);   // A_j, then acc_j
  line_t *lines = bufs.get<line_t>(ch * MILLER_LINES);
  u32 *words = bufs.get<u32>(5 * ch);                     // curve flags of A/C, of B, is_one, verdicts, status words
  fp12_t *f = bufs.get<fp12_t>((separate ? 3 : 1) * ch);
  fp12_t *ws = bufs.get<fp12_t>(4 * ch);                  // final exponentiation workspace
  KeyBlock *blk = bufs.get<KeyBlock>(max_blocks);
  unsigned char *cbytes = bytes ? bufs.get<unsigned char>(ch * 192) : nullptr;
  u32 *pst = bytes ? bufs.get<u32>(3 * ch) : nullptr;
  unsigned long long *first_bad = bytes ? bufs.get<unsigned long long>(1) : nullptr;   // (the reader's; not used here)
  if (!pr || !ind || !pts || !lines || !words || !f || !ws || !blk || (bytes && (!cbytes || !pst || !first_bad))) {
    fprintf(stderr, "[bellman_hip] verify_each_keys: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  u32 *pflags = words, *qflags = words + ch, *is_one = words + 2 * ch, *wst = bytes ? words + 4 * ch : nullptr;
  int *vd = (int *)(words + 3 * ch);
  Affine<FpOps> *accp = pts + ch;
  const size_t rec = bytes ? 192 : sizeof(ProofRec);
  const unsigned char *src = (const unsigned char *)(bytes ? bytes : proofs);
  Grouping g;
  std::vector<unsigned char> hrec, hin;
  std::vector<int32_t> hv(ch);
  std::vector<uint32_t> hs(ch);
  size_t bad = 0;
  for (size_t first = 0; first < n_proofs; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    g.make(set, key_of + first, m);
    keys_gather(g, set, key_of + first, src + first * rec, rec, (const unsigned char *)inputs, offs.data() + first, hrec, hin);
    const size_t nb = g.blocks.size();
    if (hipMemcpyAsync(blk, g.blocks.data(), nb * sizeof(KeyBlock), hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
    if (bytes) {
      if (hipMemcpyAsync(cbytes, hrec.data(), m * 192, hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
      if ((rc = proofs_read_dev(cbytes, pr, m, pst, wst, first_bad, st))) return rc;
    } else if (hipMemcpyAsync(pr, hrec.data(), m * sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) {
      return BH_ERR_HIP;
    }
    if (g.n_in && hipMemcpyAsync(ind, hin.data(), g.n_in * 32, hipMemcpyHostToDevice, st) != hipSuccess) return BH_ERR_HIP;
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, pr, (const fr_t *)nullptr, 0, pts,
                       (Affine<FpOps> *)nullptr, (fr_t *)nullptr, (const Affine<FpOps> *)nullptr, pflags, (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    if ((rc = launch_ic_accumulate_keys(st, ind, scalar_fmt, kd, blk, nb, accp))) return rc;
    if ((rc = launch_g2_lines(st, &pr->b, sizeof(ProofRec), 0, lines, qflags, m))) return rc;
    if ((rc = launch_miller3_keys(st, pts, accp, pr, lines, qflags, kd, blk, nb, separate, f, m))) return rc;
    if ((rc = launch_fold3_const_keys(st, f, kd, blk, nb, m, separate))) return rc;
    if ((rc = launch_final_exp(st, f, m, f, is_one, ws))) return rc;
    hipLaunchKernelGGL(verdict_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, st, wst, pflags, qflags, is_one, vd, (u32)m);
    if (hipGetLastError() != hipSuccess) return BH_ERR_HIP;
    if (hipMemcpyAsync(hv.data(), vd, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (status && hipMemcpyAsync(hs.data(), wst, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
      return BH_ERR_HIP;
    for (size_t r = 0; r < m; r++) {
      verdicts[first + g.perm[r]] = hv[r];
      if (status) status[first + g.perm[r]] = hs[r];
      bad += hv[r] != BH_OK;
    }
  }
  if (n_bad) *n_bad = bad;
  return BH_OK;
}

// bh_groth16_batch_verify over a set: with E_j the value whose being 1 is proof j's equation under its own key,
// prod_j E_j^{z_j} == 1 - the product over the keys of what batch_verify_impl tests per key, under ONE final
// exponentiation.  Per chunk: one column-sum launch for all keys, one multiexp job per key that has rows (issued
// together); the tail runs [acc_Y,k] alpha_k on K lanes, Psi_k per key, and ONE Miller launch over the 3 K key pairs.
int batch_verify_keys_impl(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, const void *bytes, size_t n_proofs,
                           const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z, size_t *bad_index) {
  std::vector<size_t> offs;
  int rc = keys_check_args(set, key_of, n_proofs, inputs, n_inputs_total, scalar_fmt, offs);
  if (rc) return rc;
  if (n_proofs && ((!proofs && !bytes) || !z)) return BH_ERR_INVALID_ARG;
  if (!n_proofs) return BH_OK;
  for (size_t j = 0; j < n_proofs; j++)
    if (scalar_is_zero_mod_q((const uint8_t *)z + 32 * j)) return BH_ERR_INVALID_ARG;
  bh_ctx *ctx = set->ctx;
  Context &c = ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
  const size_t nk = set->keys.size(), ncol = set->total_cols;
  const KeyDesc *kd = set->dev;
  PoolBufs bufs(c);     // declared before the stream: released only after the stream has drained
  StreamHold sh(ctx);
  if (bh_stream_create(ctx, (void **)&sh.st) != BH_OK) return BH_ERR_HIP;
  hipStream_t st = sh.st;
  const size_t ch = keys_chunk(set, n_proofs);
  size_t in_max = 1;
  for (size_t first = 0; first < n_proofs; first += ch)
    in_max = std::max(in_max, offs[std::min(first + ch, n_proofs)] - offs[first]);
  ProofRec *pr = bufs.get<ProofRec>(ch);
  fr_t *zd = bufs.get<fr_t>(ch);
  fr_t *ind = bufs.get<fr_t>(in_max);
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
  KeySeg *segd = bufs.get<KeySeg>(nk);
  fp12_t *fk = bufs.get<fp12_t>(3 * nk + 1 + 5);          // the key pairs' values, the running product, final exponentiation
  unsigned char *cbytes = bytes ? bufs.get<unsigned char>(ch * 192) : nullptr;
  u32 *pst = bytes ? bufs.get<u32>(4 * ch) : nullptr;
  unsigned long long *first_bad = bytes ? bufs.get<unsigned long long>(1) : nullptr;
  if (bytes && (!cbytes || !pst || !first_bad)) return BH_ERR_HIP;
  if (!pr || !zd || !ind || !pts || !cb || !zc || !lines || !pflags || !qflags || !f || !facc || !part || !acc || !key || !gen ||
      !segd || !fk) {
    fprintf(stderr, "[bellman_hip] batch verification over a key set: no device memory for a %zu-proof chunk\n", ch);
    return BH_ERR_HIP;
  }
  fp12_t one;
  f12_one(one);
  Affine<FpOps> gpt;
  g1_generator(gpt);
  if (hipMemcpyAsync(facc, &one, sizeof one, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(gen, &gpt, sizeof gpt, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(acc, 0, ncol * sizeof(fr_t), st) != hipSuccess)
    return BH_ERR_HIP;
  std::vector<Affine<FpOps>> sum_c(nk);   // per key: sum z_j C_j over the chunks so far (host, affine)
  memset(sum_c.data(), 0, nk * sizeof(Affine<FpOps>));
  std::vector<unsigned char> active(nk, 0);
  u32 bad = 0;
  std::vector<u32> hflags(ch), hqflags(ch), hwords(bytes ? ch : 0);
  const size_t rec = bytes ? 192 : sizeof(ProofRec);
  const unsigned char *src = (const unsigned char *)(bytes ? bytes : proofs);
  Grouping g;
  std::vector<unsigned char> hrec, hin, hz;
  std::vector<bh_bases *> cbases(nk, nullptr);
  std::vector<bh_msm_job *> jobs(nk, nullptr);
  for (size_t first = 0; first < n_proofs && !rc; first += ch) {
    const size_t m = std::min(ch, n_proofs - first);
    g.make(set, key_of + first, m);
    keys_gather(g, set, key_of + first, src + first * rec, rec, (const unsigned char *)inputs, offs.data() + first, hrec, hin);
    hz.resize(m * 32);
    for (size_t r = 0; r < m; r++) memcpy(&hz[r * 32], (const unsigned char *)z + (first + g.perm[r]) * 32, 32);
    unsigned long long hbad = ~0ULL;   // a proof of the chunk that Proof::read refuses
    if (hipMemcpyAsync(segd, g.segs.data(), nk * sizeof(KeySeg), hipMemcpyHostToDevice, st) != hipSuccess) { rc = BH_ERR_HIP; break; }
    if (bytes) {
      if (hipMemcpyAsync(cbytes, hrec.data(), m * 192, hipMemcpyHostToDevice, st) != hipSuccess ||
          hipMemsetAsync(first_bad, 0xff, 8, st) != hipSuccess) {
        rc = BH_ERR_HIP;
        break;
      }
      if ((rc = proofs_read_dev(cbytes, pr, m, pst, pst + 3 * ch, first_bad, st))) break;
      if (hipMemcpyAsync(&hbad, first_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = BH_ERR_HIP; break; }
    } else if (hipMemcpyAsync(pr, hrec.data(), m * sizeof(ProofRec), hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = BH_ERR_HIP;
      break;
    }
    if (hipMemcpyAsync(zd, hz.data(), m * 32, hipMemcpyHostToDevice, st) != hipSuccess ||
        (g.n_in && hipMemcpyAsync(ind, hin.data(), g.n_in * 32, hipMemcpyHostToDevice, st) != hipSuccess)) {
      rc = BH_ERR_HIP;
      break;
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, pr, zd, scalar_fmt, pts, cb, zc, gen, pflags,
                       (u32)m);
    if (hipGetLastError() != hipSuccess) { rc = BH_ERR_HIP; break; }
    if ((rc = launch_g2_lines(st, &pr->b, sizeof(ProofRec), 1, lines, qflags, m))) break;   // -B_j
    if ((rc = launch_colsum_keys(st, zd, ind, scalar_fmt, kd, segd, nk, set->max_in + 1, ncol, g.max_seg, part, acc))) break;
    // sum z_j C_j of every key's run on the multiexp path, ordered after the prep kernel: all issued before the first wait
    for (size_t k = 0; k < nk && !rc; k++) {
      const KeySeg &s = g.segs[k];
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
                (bytes && hipMemcpyAsync(hwords.data(), pst + 3 * ch, m * 4, hipMemcpyDeviceToHost, st) != hipSuccess)))
      rc = BH_ERR_HIP;
    std::vector<Affine<FpOps>> part_c(nk);
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
    if (hbad != ~0ULL) {   // Proof::read failed in this chunk: the first such proof in the CALLER's order
      size_t where = ~size_t(0);
      for (size_t r = 0; r < m; r++)
        if (proof_status_error(hwords[r]) != BH_OK && g.perm[r] < where) where = g.perm[r];
      if (where == ~size_t(0)) return BH_ERR_HIP;
      if (bad_index) *bad_index = first + where;
      for (size_t r = 0; r < m; r++)
        if (g.perm[r] == where) return proof_status_error(hwords[r]);
    }
    for (size_t j = 0; j < m; j++) bad |= hflags[j] | (hqflags[j] & PF_OFF_CURVE);
  }
  if (rc) return rc;
  if (bad & PF_OFF_CURVE) return BH_ERR_INVALID_POINT;
  // [acc_Y,k] alpha_k on K lanes, then Psi_k = sum acc_Gamma_{k,i} ic_{k,i} with the scalars of identity ic_i zeroed (the
  // zeroing is ordered after the read of acc_Y,k); a key without a proof in the batch takes no part (three identities)
  if ((rc = launch_g1_mul_keys(st, key + 2 * nk, kd, acc, nk))) return rc;
  for (size_t k = 0; k < nk; k++) {
    const bh_pvk *pvk = set->keys[k];
    for (size_t i = 0; i < pvk->n_ic; i++)
      if (pvk->ic_identity[i] && hipMemsetAsync(acc + set->host[k].col_off + i, 0, sizeof(fr_t), st) != hipSuccess) return BH_ERR_HIP;
  }
  for (size_t k = 0; k < nk && !rc; k++)
    if (active[k])
      rc = bh_msm_async_dev_after(ctx, set->keys[k]->ic, 0, acc + set->host[k].col_off, set->keys[k]->n_ic, BH_SCALARS_MONT, nullptr,
                                  0, nullptr, (void *)st, &jobs[k]);
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
  if ((rc = launch_miller_keys(st, key, kd, nk, fk))) return rc;
  if (hipMemcpyAsync(fk + 3 * nk, facc, sizeof(fp12_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return BH_ERR_HIP;
  if ((rc = launch_fold(st, fk, 3 * nk + 1))) return rc;
  fp12_t *fe = fk + 3 * nk + 1;
  if ((rc = launch_final_exp(st, fk, 1, fe, qflags, fe + 1))) return rc;
  u32 h = 0;
  if (hipMemcpyAsync(&h, qflags, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return BH_ERR_HIP;
  return h == 1 ? BH_OK : BH_ERR_INVALID_PROOF;
}
}  // namespace

extern "C" {

int bh_groth16_pvk_set_create(const bh_pvk *const *pvks, size_t n_keys, bh_pvk_set **out) {
  if (!pvks || !out || !n_keys || n_keys > BH_PVK_SET_MAX_KEYS) return BH_ERR_INVALID_ARG;
  for (size_t k = 0; k < n_keys; k++)
    if (!pvks[k] || pvks[k]->ctx != pvks[0]->ctx) return BH_ERR_INVALID_ARG;
  std::unique_ptr<bh_pvk_set> s(new bh_pvk_set);
  s->ctx = pvks[0]->ctx;
  Context &c = s->ctx->c;
  BH_HIP_CHECK(hipSetDevice(c.device));
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
  StreamHold sh(s->ctx);
  int rc = bh_stream_create(s->ctx, (void **)&sh.st);
  if (rc) sh.st = nullptr;
  if (!rc && (hipMemcpyAsync(s->dev, s->host.data(), n_keys * sizeof(KeyDesc), hipMemcpyHostToDevice, sh.st) != hipSuccess ||
              hipStreamSynchronize(sh.st) != hipSuccess))
    rc = BH_ERR_HIP;
  if (rc) {
    c.pool.release(s->dev);
    return rc;
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
  return verify_each_keys_impl(set, key_of, proofs, nullptr, n_proofs, inputs, n_inputs_total, scalar_fmt, verdicts, nullptr,
                               n_bad);
}

int bh_groth16_verify_each_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                           const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts,
                                           uint32_t *status, size_t *n_bad) {
  return verify_each_keys_impl(set, key_of, nullptr, bytes, n_proofs, inputs, n_inputs_total, scalar_fmt, verdicts, status, n_bad);
}

int bh_groth16_batch_verify_keys(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, size_t n_proofs,
                                 const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z) {
  return batch_verify_keys_impl(set, key_of, proofs, nullptr, n_proofs, inputs, n_inputs_total, scalar_fmt, z, nullptr);
}

int bh_groth16_batch_verify_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                            const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z,
                                            size_t *bad_index) {
  return batch_verify_keys_impl(set, key_of, nullptr, bytes, n_proofs, inputs, n_inputs_total, scalar_fmt, z, bad_index);
}

}  // extern "C"
