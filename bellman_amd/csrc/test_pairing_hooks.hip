// libbellman_hip_test.so: every kernel of the Groth16 verifier on its own (bh_test_pairing_* of include/bellman_hip_test.h;
// tests/test_gpu_pairing_stages.py, tests/models/pairing_stage_model.py).  This translation unit INCLUDES
// pairing_kernels.cuh: the kernels and the launch functions are the shipped text, compiled a second time into the test
// library; where the product launches a kernel inline (proof_prep, g1_mul_one, ic_table, ic_accumulate, miller3, verdict)
// the hook launches it with the product's block size.  Every argument is validated on the host before anything is
// launched.  Every device buffer has exactly its production size and a guard behind it; outputs and guards start filled
// with the sentinel byte, and results come back raw.
#include <string.h>

#include <vector>

#include "../../include/bellman_hip_test.h"
#include "pairing_kernels.cuh"

namespace bh {
namespace pairstage {

constexpr size_t GUARD = 4096;             // bytes behind every buffer that must come back untouched
constexpr unsigned char SENTINEL = 0xA5;   // what outputs hold before the launch
constexpr size_t MAX_N = 1 << 15;          // lanes per call
typedef Affine<FpOps> G1A;

struct DevBuf {   // `bytes` of payload + GUARD, freed on scope exit
  char *p = nullptr;
  size_t bytes = 0;
  std::vector<unsigned char> guard;
  ~DevBuf() { if (p) (void)hipFree(p); }
  // host != NULL: an input, uploaded; else an output, filled with the sentinel
  int make(size_t n, const void *host, hipStream_t st) {
    bytes = n;
    BH_HIP_CHECK(hipMalloc((void **)&p, n + GUARD));
    BH_HIP_CHECK(hipMemsetAsync(p, SENTINEL, n + GUARD, st));
    if (n && host) BH_HIP_CHECK(hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, st));
    return BH_OK;
  }
  int fetch(void *host, hipStream_t st) {
    guard.resize(GUARD);
    if (host && bytes) BH_HIP_CHECK(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, st));
    BH_HIP_CHECK(hipMemcpyAsync(guard.data(), p + bytes, GUARD, hipMemcpyDeviceToHost, st));
    return BH_OK;
  }
  u32 intact() const {
    for (unsigned char b : guard)
      if (b != SENTINEL) return 0;
    return guard.size() == GUARD;
  }
  template <class T>
  T *as() const { return (T *)p; }
};
// run `launch` between the uploads and the downloads of bufs[0..k): outs[i] (may be NULL) receives the payload of bufs[i]
template <class Launch>
static int run(Context &cx, DevBuf *const *bufs, const size_t *sizes, const void *const *ins, void *const *outs, int k,
               uint32_t *guards, Launch &&launch) {
  BH_HIP_CHECK(hipSetDevice(cx.device));
  hipStream_t st = cx.stream;
  int rc;
  for (int i = 0; i < k; i++)
    if ((rc = bufs[i]->make(sizes[i], ins[i], st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));   // (pageable host memory: the copies above may still be staged)
  if ((rc = launch(st))) return rc;
  for (int i = 0; i < k; i++)
    if ((rc = bufs[i]->fetch(outs[i], st))) return rc;
  BH_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < k; i++) guards[i] = bufs[i]->intact();
  return BH_OK;
}
static bool fmt_ok(int fmt) { return fmt == BH_SCALARS_CANONICAL || fmt == BH_SCALARS_MONT; }
static bool width_ok(unsigned w) { return w == 1 || w == 2 || w == 4 || w == 8; }
static size_t table_entries(size_t n_in, unsigned w) { return n_in * (256 / w) * ((size_t(1) << w) - 1); }

}  // namespace pairstage
}  // namespace bh

using namespace bh;
using namespace bh::pairstage;

#define BH_STAGE_RUN(K, LAUNCH) run(ctx->c, bufs, sizes, ins, outs, K, guards, [&](hipStream_t st) -> int LAUNCH)

extern "C" {

int bh_test_pairing_stage_shape(uint64_t out16[16]) {
  if (!out16) return BH_ERR_INVALID_ARG;
  const uint64_t v[16] = {sizeof(line_t), sizeof(fp12_t), sizeof(ProofRec), (uint64_t)MILLER_LINES, PF_IDENTITY, PF_OFF_CURVE,
                          PT_INVALID_MASK, PT_IS_INF, COLSUM_THREADS, COLSUM_BLOCKS, BATCH_CHUNK, GUARD, SENTINEL,
                          offsetof(ProofRec, b), offsetof(ProofRec, c), sizeof(G1A)};
  memcpy(out16, v, sizeof v);
  return BH_OK;
}

// host only: the shipped proof_status_error (csrc/points.hpp) of a status word
int bh_test_proof_status_error(uint32_t word) { return proof_status_error(word); }

int bh_test_pairing_lines_dev(bh_ctx *ctx, const void *records, size_t stride_bytes, int negate, size_t n, void *lines_out,
                              uint32_t *flags_out, uint32_t guards[3]) {
  if (!ctx || !records || !lines_out || !flags_out || !guards || !n || n > MAX_N) return BH_ERR_INVALID_ARG;
  if (stride_bytes != sizeof(Affine<Fp2Ops>) && stride_bytes != sizeof(ProofRec)) return BH_ERR_INVALID_ARG;
  const size_t off = stride_bytes == sizeof(ProofRec) ? offsetof(ProofRec, b) : 0;
  DevBuf q, lines, flags;
  DevBuf *bufs[] = {&q, &lines, &flags};
  const size_t sizes[] = {n * stride_bytes, n * MILLER_LINES * sizeof(line_t), n * 4};
  const void *ins[] = {records, nullptr, nullptr};
  void *outs[] = {nullptr, lines_out, flags_out};
  return BH_STAGE_RUN(3, { return launch_g2_lines(st, q.p + off, stride_bytes, negate, lines.as<line_t>(), flags.as<u32>(), n); });
}

int bh_test_pairing_miller_dev(bh_ctx *ctx, const void *p, const void *lines0, const uint32_t *flags0, size_t n0,
                               const void *lines1, const uint32_t *flags1, size_t n1, void *f_out, uint32_t guards[6]) {
  const size_t n = n0 + n1;
  if (!ctx || !p || !f_out || !guards || !n || n > MAX_N || (n0 && (!lines0 || !flags0)) || (n1 && (!lines1 || !flags1)))
    return BH_ERR_INVALID_ARG;
  static const char none = 0;
  DevBuf dp, l0, f0, l1, f1, f;
  DevBuf *bufs[] = {&dp, &l0, &f0, &l1, &f1, &f};
  const size_t sizes[] = {n * sizeof(G1A), n0 * MILLER_LINES * sizeof(line_t), n0 * 4, n1 * MILLER_LINES * sizeof(line_t), n1 * 4,
                          n * sizeof(fp12_t)};
  const void *ins[] = {p, n0 ? lines0 : &none, n0 ? (const void *)flags0 : &none, n1 ? lines1 : &none,
                       n1 ? (const void *)flags1 : &none, nullptr};
  void *outs[] = {nullptr, nullptr, nullptr, nullptr, nullptr, f_out};
  return BH_STAGE_RUN(6, {
    return launch_miller(st, dp.as<G1A>(), l0.as<line_t>(), f0.as<u32>(), f.as<fp12_t>(), n0, l1.as<line_t>(), f1.as<u32>(), n1);
  });
}

int bh_test_pairing_fold_dev(bh_ctx *ctx, void *f_inout, size_t m, uint32_t guards[1]) {
  if (!ctx || !f_inout || !guards || !m || m > MAX_N) return BH_ERR_INVALID_ARG;
  DevBuf f;
  DevBuf *bufs[] = {&f};
  const size_t sizes[] = {m * sizeof(fp12_t)};
  const void *ins[] = {f_inout};
  void *outs[] = {f_inout};
  return BH_STAGE_RUN(1, { return launch_fold(st, f.as<fp12_t>(), m); });
}

int bh_test_pairing_proof_prep_dev(bh_ctx *ctx, const void *proofs, const void *z, int fmt, size_t n, int want_c,
                                   const void *g1_generator, void *p_out, void *c_out, void *zc_out, uint32_t *flags_out,
                                   uint32_t guards[7]) {
  if (!ctx || !proofs || !p_out || !flags_out || !guards || !n || n > MAX_N || !fmt_ok(fmt)) return BH_ERR_INVALID_ARG;
  if (want_c && (!g1_generator || !c_out || !zc_out)) return BH_ERR_INVALID_ARG;
  static const char none = 0;
  DevBuf pr, dz, gen, po, co, zo, fl;
  DevBuf *bufs[] = {&pr, &dz, &gen, &po, &co, &zo, &fl};
  const size_t sizes[] = {n * sizeof(ProofRec), z ? n * 32 : 0, want_c ? sizeof(G1A) : 0, n * sizeof(G1A),
                          want_c ? n * sizeof(G1A) : 0, want_c ? n * 32 : 0, n * 4};
  const void *ins[] = {proofs, z ? z : &none, want_c ? g1_generator : &none, nullptr, nullptr, nullptr, nullptr};
  void *outs[] = {nullptr, nullptr, nullptr, p_out, want_c ? c_out : nullptr, want_c ? zc_out : nullptr, flags_out};
  return BH_STAGE_RUN(7, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(proof_prep_kernel, dim3(blocks_of(n, 64)), dim3(64), 0, st, pr.as<ProofRec>(), z ? dz.as<fr_t>() : nullptr,
                       fmt, po.as<G1A>(), want_c ? co.as<G1A>() : nullptr, want_c ? zo.as<fr_t>() : nullptr,
                       want_c ? gen.as<G1A>() : nullptr, fl.as<u32>(), (u32)n);
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

int bh_test_pairing_g1_mul_one_dev(bh_ctx *ctx, const void *p, const void *s_mont, void *out, uint32_t guards[3]) {
  if (!ctx || !p || !s_mont || !out || !guards) return BH_ERR_INVALID_ARG;
  DevBuf dp, ds, o;
  DevBuf *bufs[] = {&dp, &ds, &o};
  const size_t sizes[] = {sizeof(G1A), 32, sizeof(G1A)};
  const void *ins[] = {p, s_mont, nullptr};
  void *outs[] = {nullptr, nullptr, out};
  return BH_STAGE_RUN(3, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(g1_mul_one_kernel, dim3(1), dim3(64), 0, st, o.as<G1A>(), dp.as<G1A>(), ds.as<fr_t>());
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

int bh_test_pairing_colsum_dev(bh_ctx *ctx, const void *z, const void *inputs, size_t n_inputs, int fmt, size_t n,
                               unsigned nb_override, void *acc_inout, void *part_out, uint32_t guards[4]) {
  if (!ctx || !z || !acc_inout || !part_out || !guards || !n || n > BATCH_CHUNK || n_inputs > 1024 || (n_inputs && !inputs) ||
      !fmt_ok(fmt) || nb_override > COLSUM_BLOCKS)
    return BH_ERR_INVALID_ARG;
  static const char none = 0;
  const size_t ncol = n_inputs + 1;
  DevBuf dz, in, part, acc;
  DevBuf *bufs[] = {&dz, &in, &part, &acc};
  const size_t sizes[] = {n * 32, n * n_inputs * 32, ncol * COLSUM_BLOCKS * 32, ncol * 32};
  const void *ins[] = {z, n_inputs ? inputs : &none, nullptr, acc_inout};
  void *outs[] = {nullptr, nullptr, part_out, acc_inout};
  return BH_STAGE_RUN(4, {
    return launch_colsum(st, dz.as<fr_t>(), in.as<fr_t>(), n_inputs, fmt, n, part.as<fr_t>(), acc.as<fr_t>(), nb_override);
  });
}

int bh_test_pairing_ic_table_dev(bh_ctx *ctx, const void *ic, size_t n_in, unsigned w, void *table_out, uint32_t guards[2]) {
  if (!ctx || !ic || !table_out || !guards || !n_in || n_in > 64 || !width_ok(w)) return BH_ERR_INVALID_ARG;
  const size_t total = table_entries(n_in, w);
  DevBuf dic, tab;
  DevBuf *bufs[] = {&dic, &tab};
  const size_t sizes[] = {n_in * sizeof(G1A), total * sizeof(G1A)};
  const void *ins[] = {ic, nullptr};
  void *outs[] = {nullptr, table_out};
  return BH_STAGE_RUN(2, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(ic_table_kernel, dim3(blocks_of(total, 64)), dim3(64), 0, st, dic.as<G1A>(), w, tab.as<G1A>(), (u32)total);
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

int bh_test_pairing_ic_accumulate_dev(bh_ctx *ctx, const void *inputs, size_t n_inputs, int fmt, const void *table, unsigned w,
                                      const void *ic0, size_t n, void *out, uint32_t guards[4]) {
  if (!ctx || !ic0 || !out || !guards || !n || n > MAX_N || n_inputs > 64 || (n_inputs && (!inputs || !table)) || !fmt_ok(fmt) ||
      !width_ok(w))
    return BH_ERR_INVALID_ARG;
  static const char none = 0;
  DevBuf in, tab, d0, o;
  DevBuf *bufs[] = {&in, &tab, &d0, &o};
  const size_t sizes[] = {n * n_inputs * 32, table_entries(n_inputs, w) * sizeof(G1A), sizeof(G1A), n * sizeof(G1A)};
  const void *ins[] = {n_inputs ? inputs : &none, n_inputs ? table : &none, ic0, nullptr};
  void *outs[] = {nullptr, nullptr, nullptr, out};
  return BH_STAGE_RUN(4, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(ic_accumulate_kernel, dim3(blocks_of(n, 64)), dim3(64), 0, st, in.as<fr_t>(), (u32)n_inputs, fmt,
                       n_inputs ? tab.as<G1A>() : nullptr, w, d0.as<G1A>(), o.as<G1A>(), (u32)n);
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

int bh_test_pairing_miller3_dev(bh_ctx *ctx, const void *a, const void *acc, const void *proofs, const void *blines,
                                const uint32_t *bflags, const void *klines, const uint32_t *kflags2, int separate, unsigned pairs,
                                size_t n, void *f_out, uint32_t guards[8]) {
  if (!ctx || !a || !acc || !proofs || !blines || !bflags || !klines || !kflags2 || !f_out || !guards || !n || n > MAX_N ||
      pairs > 7u)
    return BH_ERR_INVALID_ARG;
  DevBuf da, dg, pr, bl, bf, kl, kf, f;
  DevBuf *bufs[] = {&da, &dg, &pr, &bl, &bf, &kl, &kf, &f};
  const size_t sizes[] = {n * sizeof(G1A), n * sizeof(G1A), n * sizeof(ProofRec), n * MILLER_LINES * sizeof(line_t), n * 4,
                          2 * MILLER_LINES * sizeof(line_t), 8, (separate ? 3 : 1) * n * sizeof(fp12_t)};
  const void *ins[] = {a, acc, proofs, blines, bflags, klines, kflags2, nullptr};
  void *outs[] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, f_out};
  return BH_STAGE_RUN(8, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(miller3_kernel, dim3(blocks_of(n, 64), separate ? 3 : 1), dim3(64), 0, st, da.as<G1A>(), dg.as<G1A>(),
                       pr.as<ProofRec>(), bl.as<line_t>(), bf.as<u32>(), kl.as<line_t>(), kf.as<u32>(), pairs, f.as<fp12_t>(), (u32)n);
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

int bh_test_pairing_fold3_const_dev(bh_ctx *ctx, void *f_inout, const void *c, size_t n, int separate, uint32_t guards[2]) {
  if (!ctx || !f_inout || !c || !guards || !n || n > MAX_N) return BH_ERR_INVALID_ARG;
  DevBuf f, dc;
  DevBuf *bufs[] = {&f, &dc};
  const size_t sizes[] = {(separate ? 3 : 1) * n * sizeof(fp12_t), sizeof(fp12_t)};
  const void *ins[] = {f_inout, c};
  void *outs[] = {f_inout, nullptr};
  return BH_STAGE_RUN(2, { return launch_fold3_const(st, f.as<fp12_t>(), dc.as<fp12_t>(), n, separate != 0); });
}

int bh_test_pairing_verdict_dev(bh_ctx *ctx, const uint32_t *words, const uint32_t *pflags, const uint32_t *qflags,
                                const uint32_t *is_one, size_t n, int32_t *verdicts_out, uint32_t guards[5]) {
  if (!ctx || !pflags || !qflags || !is_one || !verdicts_out || !guards || !n || n > MAX_N) return BH_ERR_INVALID_ARG;
  static const char none = 0;
  DevBuf w, pf, qf, io, v;
  DevBuf *bufs[] = {&w, &pf, &qf, &io, &v};
  const size_t sizes[] = {words ? n * 4 : 0, n * 4, n * 4, n * 4, n * 4};
  const void *ins[] = {words ? (const void *)words : &none, pflags, qflags, is_one, nullptr};
  void *outs[] = {nullptr, nullptr, nullptr, nullptr, verdicts_out};
  return BH_STAGE_RUN(5, {
    (void)hipGetLastError();
    hipLaunchKernelGGL(verdict_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, words ? w.as<u32>() : nullptr, pf.as<u32>(),
                       qf.as<u32>(), io.as<u32>(), (int *)v.p, (u32)n);
    BH_HIP_CHECK(hipGetLastError());
    return BH_OK;
  });
}

// ---- the key-aware kernels (bh_groth16_*_keys): the keys of a set as bh_test_key_layout names them, uploaded as seven
// buffers (tables, ic_0, lines, flags, f(-alpha, beta), alpha, the descriptors), whose guards follow the hook's own
struct KeyBufs {
  DevBuf tables, ic0, lines, qflags, fab, alpha, descs;
  std::vector<size_t> table_off;   // records before key k's table
  size_t total_cols = 0, max_in = 0, table_total = 0;
  bool check(const bh_test_key_layout *k, bool tables_needed) {
    if (!k || !k->n_keys || k->n_keys > BH_PVK_SET_MAX_KEYS || !k->n_inputs || !k->widths) return false;
    table_off.assign(k->n_keys, 0);
    for (size_t i = 0; i < k->n_keys; i++) {
      if (k->n_inputs[i] > 64 || !width_ok(k->widths[i])) return false;
      table_off[i] = table_total;
      table_total += table_entries(k->n_inputs[i], k->widths[i]);
      total_cols += k->n_inputs[i] + 1;
      max_in = std::max<size_t>(max_in, k->n_inputs[i]);
    }
    return !(tables_needed && table_total && !k->tables);
  }
  // appends the seven buffers to the hook's lists from position `at` on
  void list(const bh_test_key_layout *k, DevBuf **bufs, size_t *sizes, const void **ins, void **outs, int at) {
    static const char none = 0;
    const size_t nk = k->n_keys;
    DevBuf *b[7] = {&tables, &ic0, &lines, &qflags, &fab, &alpha, &descs};
    const size_t sz[7] = {k->tables ? table_total * sizeof(G1A) : 0, k->ic0 ? nk * sizeof(G1A) : 0,
                          k->lines ? nk * 3 * MILLER_LINES * sizeof(line_t) : 0, k->qflags ? nk * 12 : 0,
                          k->f_ab ? nk * sizeof(fp12_t) : 0, k->alpha ? nk * sizeof(G1A) : 0, nk * sizeof(KeyDesc)};
    const void *in[7] = {k->tables, k->ic0, k->lines, k->qflags, k->f_ab, k->alpha, nullptr};
    for (int i = 0; i < 7; i++) {
      bufs[at + i] = b[i];
      sizes[at + i] = sz[i];
      ins[at + i] = sz[i] && in[i] ? in[i] : (i == 6 ? nullptr : &none);
      outs[at + i] = nullptr;
    }
  }
  // the descriptors over the uploaded buffers, written before the launch
  int write_descs(const bh_test_key_layout *k, hipStream_t st) {
    std::vector<KeyDesc> d(k->n_keys);
    u32 col = 0;
    for (size_t i = 0; i < k->n_keys; i++) {
      memset(&d[i], 0, sizeof(KeyDesc));
      d[i].lines = k->lines ? lines.as<line_t>() + i * 3 * MILLER_LINES : nullptr;
      d[i].qflags = k->qflags ? qflags.as<u32>() + 3 * i : nullptr;
      d[i].alpha = k->alpha ? alpha.as<G1A>() + i : nullptr;
      d[i].table = k->tables && k->n_inputs[i] ? tables.as<G1A>() + table_off[i] : nullptr;
      d[i].ic0 = k->ic0 ? ic0.as<G1A>() + i : nullptr;
      d[i].f_ab = k->f_ab ? fab.as<fp12_t>() + i : nullptr;
      d[i].w = k->widths[i];
      d[i].n_inputs = k->n_inputs[i];
      d[i].col_off = col;
      col += k->n_inputs[i] + 1;
    }
    BH_HIP_CHECK(hipMemcpyAsync(descs.p, d.data(), d.size() * sizeof(KeyDesc), hipMemcpyHostToDevice, st));
    BH_HIP_CHECK(hipStreamSynchronize(st));
    return BH_OK;
  }
};
// every block inside the chunk's n rows and n_scalars inputs, of an existing key, with 1 .. 64 rows
static bool blocks_ok(const bh_test_key_layout *k, const uint32_t *blocks, size_t nblocks, size_t n, size_t n_scalars) {
  if (!blocks || !nblocks || nblocks > MAX_N) return false;
  for (size_t b = 0; b < nblocks; b++) {
    const uint32_t key = blocks[4 * b], first = blocks[4 * b + 1], count = blocks[4 * b + 2], in_off = blocks[4 * b + 3];
    if (key >= k->n_keys || !count || count > 64 || (size_t)first + count > n) return false;
    if ((size_t)in_off + (size_t)count * k->n_inputs[key] > n_scalars) return false;
  }
  return true;
}

int bh_test_pairing_ic_accumulate_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                           const void *inputs, size_t n_scalars, int fmt, size_t n, void *out, uint32_t guards[10]) {
  KeyBufs kb;
  if (!ctx || !out || !guards || !n || n > MAX_N || !fmt_ok(fmt) || (n_scalars && !inputs) || !kb.check(keys, true) || !keys->ic0 ||
      !blocks_ok(keys, blocks, nblocks, n, n_scalars))
    return BH_ERR_INVALID_ARG;
  static const char none = 0;
  DevBuf in, blk, o;
  DevBuf *bufs[10] = {&in, &blk, &o};
  size_t sizes[10] = {n_scalars * 32, nblocks * sizeof(KeyBlock), n * sizeof(G1A)};
  const void *ins[10] = {n_scalars ? inputs : &none, blocks, nullptr};
  void *outs[10] = {nullptr, nullptr, out};
  kb.list(keys, bufs, sizes, ins, outs, 3);
  return BH_STAGE_RUN(10, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_ic_accumulate_keys(st, in.as<fr_t>(), fmt, kb.descs.as<KeyDesc>(), blk.as<KeyBlock>(), nblocks, o.as<G1A>());
  });
}

int bh_test_pairing_miller3_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                     const void *a, const void *acc, const void *proofs, const void *blines,
                                     const uint32_t *bflags, int separate, size_t n, void *f_out, uint32_t guards[14]) {
  KeyBufs kb;
  if (!ctx || !a || !acc || !proofs || !blines || !bflags || !f_out || !guards || !n || n > MAX_N || !kb.check(keys, false) ||
      !keys->lines || !keys->qflags || !blocks_ok(keys, blocks, nblocks, n, ~size_t(0) >> 8))
    return BH_ERR_INVALID_ARG;
  DevBuf da, dg, pr, bl, bf, blk, f;
  DevBuf *bufs[14] = {&da, &dg, &pr, &bl, &bf, &blk, &f};
  size_t sizes[14] = {n * sizeof(G1A), n * sizeof(G1A), n * sizeof(ProofRec), n * MILLER_LINES * sizeof(line_t), n * 4,
                      nblocks * sizeof(KeyBlock), (separate ? 3 : 1) * n * sizeof(fp12_t)};
  const void *ins[14] = {a, acc, proofs, blines, bflags, blocks, nullptr};
  void *outs[14] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, f_out};
  kb.list(keys, bufs, sizes, ins, outs, 7);
  return BH_STAGE_RUN(14, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_miller3_keys(st, da.as<G1A>(), dg.as<G1A>(), pr.as<ProofRec>(), bl.as<line_t>(), bf.as<u32>(),
                               kb.descs.as<KeyDesc>(), blk.as<KeyBlock>(), nblocks, separate != 0, f.as<fp12_t>(), n);
  });
}

int bh_test_pairing_fold3_const_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                         void *f_inout, size_t n, int separate, uint32_t guards[9]) {
  KeyBufs kb;
  if (!ctx || !f_inout || !guards || !n || n > MAX_N || !kb.check(keys, false) || !keys->f_ab ||
      !blocks_ok(keys, blocks, nblocks, n, ~size_t(0) >> 8))
    return BH_ERR_INVALID_ARG;
  DevBuf f, blk;
  DevBuf *bufs[9] = {&f, &blk};
  size_t sizes[9] = {(separate ? 3 : 1) * n * sizeof(fp12_t), nblocks * sizeof(KeyBlock)};
  const void *ins[9] = {f_inout, blocks};
  void *outs[9] = {f_inout, nullptr};
  kb.list(keys, bufs, sizes, ins, outs, 2);
  return BH_STAGE_RUN(9, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_fold3_const_keys(st, f.as<fp12_t>(), kb.descs.as<KeyDesc>(), blk.as<KeyBlock>(), nblocks, n, separate != 0);
  });
}

int bh_test_pairing_colsum_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *segs, const void *z,
                                    const void *inputs, size_t n_scalars, int fmt, size_t n, unsigned nb_override, void *acc_inout,
                                    void *part_out, uint32_t guards[12]) {
  KeyBufs kb;
  if (!ctx || !segs || !z || !acc_inout || !part_out || !guards || !n || n > BATCH_CHUNK || (n_scalars && !inputs) || !fmt_ok(fmt) ||
      nb_override > COLSUM_BLOCKS || !kb.check(keys, false))
    return BH_ERR_INVALID_ARG;
  size_t max_seg = 0;
  for (size_t k = 0; k < keys->n_keys; k++) {
    const uint32_t first = segs[4 * k], count = segs[4 * k + 1], in_off = segs[4 * k + 2];
    if ((size_t)first + count > n || (size_t)in_off + (size_t)count * keys->n_inputs[k] > n_scalars) return BH_ERR_INVALID_ARG;
    max_seg = std::max<size_t>(max_seg, count);
  }
  static const char none = 0;
  DevBuf dz, in, sg, part, acc;
  DevBuf *bufs[12] = {&dz, &in, &sg, &part, &acc};
  size_t sizes[12] = {n * 32, n_scalars * 32, keys->n_keys * sizeof(KeySeg), kb.total_cols * COLSUM_BLOCKS * 32, kb.total_cols * 32};
  const void *ins[12] = {z, n_scalars ? inputs : &none, segs, nullptr, acc_inout};
  void *outs[12] = {nullptr, nullptr, nullptr, part_out, acc_inout};
  kb.list(keys, bufs, sizes, ins, outs, 5);
  return BH_STAGE_RUN(12, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_colsum_keys(st, dz.as<fr_t>(), in.as<fr_t>(), fmt, kb.descs.as<KeyDesc>(), sg.as<KeySeg>(), keys->n_keys,
                              kb.max_in + 1, kb.total_cols, max_seg, part.as<fr_t>(), acc.as<fr_t>(), nb_override);
  });
}

int bh_test_pairing_g1_mul_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const void *acc_mont, void *out,
                                    uint32_t guards[9]) {
  KeyBufs kb;
  if (!ctx || !acc_mont || !out || !guards || !kb.check(keys, false) || !keys->alpha) return BH_ERR_INVALID_ARG;
  DevBuf acc, o;
  DevBuf *bufs[9] = {&acc, &o};
  size_t sizes[9] = {kb.total_cols * 32, keys->n_keys * sizeof(G1A)};
  const void *ins[9] = {acc_mont, nullptr};
  void *outs[9] = {nullptr, out};
  kb.list(keys, bufs, sizes, ins, outs, 2);
  return BH_STAGE_RUN(9, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_g1_mul_keys(st, o.as<G1A>(), kb.descs.as<KeyDesc>(), acc.as<fr_t>(), keys->n_keys);
  });
}

int bh_test_pairing_miller_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const void *p, void *f_out, uint32_t guards[9]) {
  KeyBufs kb;
  if (!ctx || !p || !f_out || !guards || !kb.check(keys, false) || !keys->lines || !keys->qflags) return BH_ERR_INVALID_ARG;
  DevBuf dp, f;
  DevBuf *bufs[9] = {&dp, &f};
  size_t sizes[9] = {3 * keys->n_keys * sizeof(G1A), 3 * keys->n_keys * sizeof(fp12_t)};
  const void *ins[9] = {p, nullptr};
  void *outs[9] = {nullptr, f_out};
  kb.list(keys, bufs, sizes, ins, outs, 2);
  return BH_STAGE_RUN(9, {
    const int rc = kb.write_descs(keys, st);
    if (rc) return rc;
    return launch_miller_keys(st, dp.as<G1A>(), kb.descs.as<KeyDesc>(), keys->n_keys, f.as<fp12_t>());
  });
}

int bh_test_pairing_final_exp_dev(bh_ctx *ctx, const void *f, size_t n, void *out, uint32_t *is_one_out, uint32_t guards[4]) {
  if (!ctx || !f || !out || !is_one_out || !guards || !n || n > 4096) return BH_ERR_INVALID_ARG;
  DevBuf df, o, io, ws;
  DevBuf *bufs[] = {&df, &o, &io, &ws};
  const size_t sizes[] = {n * sizeof(fp12_t), n * sizeof(fp12_t), n * 4, 4 * n * sizeof(fp12_t)};
  const void *ins[] = {f, nullptr, nullptr, nullptr};
  void *outs[] = {nullptr, out, is_one_out, nullptr};
  return BH_STAGE_RUN(4, { return launch_final_exp(st, df.as<fp12_t>(), n, o.as<fp12_t>(), io.as<u32>(), ws.as<fp12_t>()); });
}

}  // extern "C"
