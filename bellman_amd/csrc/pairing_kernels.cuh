// The device half of the Groth16 verifier (pairing.hip holds the host half and the description of the whole): the curve
// tests, the thirteen kernels of the one-key calls, the six key-aware ones of the calls over a key set, and the functions
// that launch them.  Included by pairing.hip (the product) and by test_pairing_hooks.hip (the test library), which runs
// every kernel on its own: tests/test_gpu_pairing_stages.py, tests/test_gpu_verify_keys_stages.py.
// ONE translation unit per library may include this header: the kernels and the launch_* functions other units call
// (pairing_launch.hpp) have external linkage, so a second including unit in the same library would define them twice.
// Another unit of the same library that needs one of those includes pairing_launch.hpp (ceremony.hip; test_hooks.hip
// for bh_test_pairing).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "final_exp.cuh"
#include "fp12.cuh"
#include "pairing_launch.hpp"
#include "points.hpp"

namespace bh {

// (PF_IDENTITY, PF_OFF_CURVE and BATCH_CHUNK: fp12.cuh, shared with ceremony.hip; on_curve: ec.cuh)
static constexpr size_t INPUTS_CHUNK_BYTES = size_t(256) << 20;

// a 32-byte scalar in the format of bh_msm_async, as a canonical 256-bit integer (a value >= q is used as is: the points
// it multiplies have order q)
BH_HD void scalar_bits(fr_t &k, const fr_t &s, int fmt) {
  if (fmt == BH_SCALARS_MONT) fe_from_mont(k, s);
  else k = s;
}

// 1. lines of Q (or -Q with negate); flags: PF_IDENTITY, PF_OFF_CURVE
__global__ __launch_bounds__(64) void g2_lines_kernel(const Affine<Fp2Ops> *q, size_t stride_words, int negate, line_t *lines,
                                                      u32 *flags, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<Fp2Ops> p = *(const Affine<Fp2Ops> *)((const u32 *)q + (size_t)i * stride_words);
  line_t *out = lines + (size_t)i * MILLER_LINES;
  if (aff_is_identity(p)) {
    flags[i] = PF_IDENTITY;
    return;
  }
  flags[i] = on_curve(p) ? 0u : PF_OFF_CURVE;
  if (negate) Fp2Ops::neg(p.y, p.y);
  g2_lines(p.x, p.y, [&](int k, const line_t &l) { out[k] = l; });
}

// 2. per proof (384-byte records a | b | c): flags of A and C, P_j = [z_j] A (z == NULL: A itself), the C base (the
// generator with a zero scalar where C is the identity: multiexp bases must not be the identity) and its scalar
struct ProofRec {
  Affine<FpOps> a;
  Affine<Fp2Ops> b;
  Affine<FpOps> c;
};
__global__ __launch_bounds__(64) void proof_prep_kernel(const ProofRec *proofs, const fr_t *z, int fmt, Affine<FpOps> *p_out,
                                                        Affine<FpOps> *c_out, fr_t *zc_out, const Affine<FpOps> *g1, u32 *flags,
                                                        u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<FpOps> a = proofs[i].a, c = proofs[i].c;
  u32 fl = 0;
  if (!aff_is_identity(a) && !on_curve(a)) fl |= PF_OFF_CURVE;
  if (!aff_is_identity(c) && !on_curve(c)) fl |= PF_OFF_CURVE;
  flags[i] = fl;
  if (c_out) {
    const bool ci = aff_is_identity(c);
    c_out[i] = ci ? *g1 : c;
    fr_t zz;
    if (ci) fe_zero(zz);
    else if (z) zz = z[i];
    else { fe_zero(zz); zz.l[0] = 1; }   // (not used by the single verification)
    zc_out[i] = zz;
  }
  if (!z) {
    p_out[i] = a;
    return;
  }
  fr_t k;
  scalar_bits(k, z[i], fmt);
  XYZZ<FpOps> acc;
  xyzz_set_identity(acc);
  if (!aff_is_identity(a))
    for (int bit = 255; bit >= 0; bit--) {
      XYZZ<FpOps> t;
      xyzz_dbl(t, acc);
      acc = t;
      if ((k.l[bit >> 5] >> (bit & 31)) & 1) xyzz_madd(acc, a);
    }
  Affine<FpOps> r;
  xyzz_to_affine(r, acc);
  p_out[i] = r;
}

// [s] P for one point and a device scalar (Montgomery): alpha * acc_Y of the batch check
__global__ __launch_bounds__(64) void g1_mul_one_kernel(Affine<FpOps> *out, const Affine<FpOps> *p, const fr_t *s) {
  if (threadIdx.x != 0) return;
  fr_t k;
  fe_from_mont(k, *s);
  const Affine<FpOps> a = *p;
  XYZZ<FpOps> acc;
  xyzz_set_identity(acc);
  if (!aff_is_identity(a))
    for (int bit = 255; bit >= 0; bit--) {
      XYZZ<FpOps> t;
      xyzz_dbl(t, acc);
      acc = t;
      if ((k.l[bit >> 5] >> (bit & 31)) & 1) xyzz_madd(acc, a);
    }
  Affine<FpOps> r;
  xyzz_to_affine(r, acc);
  *out = r;
}

// 3. column sums: part[col * nb + block] = sum over the block's proofs of z_j * a_{j,col} (a_{j,0} = 1), Montgomery
static constexpr u32 COLSUM_THREADS = 256, COLSUM_BLOCKS = 64;
BH_HD void scalar_mont(fr_t &r, const fr_t &s, int fmt) {
  if (fmt == BH_SCALARS_MONT) {
    r = s;
    return;
  }
  fe_to_mont(r, s);   // a value < 2^256 times R^2 < q R: the product is reduced
}
__global__ __launch_bounds__(COLSUM_THREADS) void fr_colsum_kernel(const fr_t *z, const fr_t *inputs, u32 n_inputs, int fmt,
                                                                   u32 n, fr_t *part) {
  __shared__ fr_t sh[COLSUM_THREADS];
  const u32 col = blockIdx.x, t = threadIdx.x;
  fr_t acc;
  fe_zero(acc);
  for (u32 j = blockIdx.y * COLSUM_THREADS + t; j < n; j += gridDim.y * COLSUM_THREADS) {
    fr_t zm, term;
    scalar_mont(zm, z[j], fmt);
    if (col == 0) term = zm;
    else {
      fr_t a;
      scalar_mont(a, inputs[(size_t)j * n_inputs + col - 1], fmt);
      fe_mul(term, zm, a);
    }
    fe_add(acc, acc, term);
  }
  sh[t] = acc;
  __syncthreads();
  for (u32 h = COLSUM_THREADS / 2; h; h >>= 1) {
    if (t < h) {
      fr_t s;
      fe_add(s, sh[t], sh[t + h]);
      sh[t] = s;
    }
    __syncthreads();
  }
  if (t == 0) part[(size_t)col * gridDim.y + blockIdx.y] = sh[0];
}
// acc[col] += sum of the column's nb partial sums
__global__ __launch_bounds__(64) void fr_colsum_finish_kernel(const fr_t *part, u32 nb, u32 ncol, fr_t *acc) {
  const u32 col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncol) return;
  fr_t s = acc[col];
  for (u32 b = 0; b < nb; b++) fe_add(s, s, part[(size_t)col * nb + b]);
  acc[col] = s;
}

// 4. Miller loops: f[j] = f_{|x|,Q_j}(P_j); the lines of Q_j at lines0 + j * 68 for j < n0, else at lines1 + (j - n0) * 68
// (a proof's own pairs and the prepared key's in one launch); an identity P or Q gives 1
__global__ __launch_bounds__(64) void miller_kernel(const Affine<FpOps> *p, const line_t *lines0, const u32 *qflags0, u32 n0,
                                                    const line_t *lines1, const u32 *qflags1, fp12_t *f, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<FpOps> pp = p[i];
  const line_t *l = i < n0 ? lines0 + (size_t)i * MILLER_LINES : lines1 + (size_t)(i - n0) * MILLER_LINES;
  const u32 qf = i < n0 ? qflags0[i] : qflags1[i - n0];
  fp12_t r;
  if (aff_is_identity(pp) || (qf & PF_IDENTITY)) {
    f12_one(r);
  } else {
    miller_loop_lines(r, pp.x, pp.y, [&](int k) { return l[k]; });
  }
  f[i] = r;
}

// 5. f[i] *= f[i + h] for i < m - h
__global__ __launch_bounds__(64) void f12_fold_kernel(fp12_t *f, u32 m, u32 h) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i + h >= m) return;
  fp12_t a = f[i], b = f[i + h];
  f12_mul(a, a, b);
  f[i] = a;
}

// ---- per-proof verdicts (bh_groth16_verify_each): one lane per proof from the inputs to the verdict --------------------
// 6. The window table of the key's ic_1 .. ic_n: entry (i, win, d - 1) = [d 2^(w win)] ic_{i+1} for d = 1 .. 2^w - 1,
// affine; one lane per entry (double-and-add over the w (win + 1) bits of the multiplier, one inversion).  The entries of
// an identity ic_i are identity records, which the accumulation skips.
__global__ __launch_bounds__(64) void ic_table_kernel(const Affine<FpOps> *ic, u32 w, Affine<FpOps> *table, u32 total) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const u32 entries = (1u << w) - 1, windows = 256 / w;
  const u32 d = t % entries + 1, win = (t / entries) % windows, i = t / (entries * windows);
  const Affine<FpOps> a = ic[i];
  XYZZ<FpOps> acc;
  xyzz_set_identity(acc);
  if (!aff_is_identity(a))
    for (int bit = (int)(w * win + w) - 1; bit >= 0; bit--) {
      XYZZ<FpOps> dd;
      xyzz_dbl(dd, acc);
      acc = dd;
      const int b = bit - (int)(w * win);
      if (b >= 0 && ((d >> b) & 1)) xyzz_madd(acc, a);
    }
  Affine<FpOps> r;
  xyzz_to_affine(r, acc);
  table[t] = r;
}
// 7. acc_j = ic_0 + sum_i a_{j,i} ic_{i+1} (verifier.rs:31-35) from the table: 256 / w mixed additions per input and no
// doubling, one inversion to affine.  xyzz_madd covers equal and opposite operands, so any inputs are summed exactly.
__global__ __launch_bounds__(64) void ic_accumulate_kernel(const fr_t *inputs, u32 n_inputs, int fmt, const Affine<FpOps> *table,
                                                           u32 w, const Affine<FpOps> *ic0, Affine<FpOps> *out, u32 n) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u32 entries = (1u << w) - 1, windows = 256 / w;
  XYZZ<FpOps> acc;
  xyzz_set_identity(acc);
#pragma unroll 1
  for (u32 i = 0; i < n_inputs; i++) {
    fr_t k;
    scalar_bits(k, inputs[(size_t)j * n_inputs + i], fmt);
    const Affine<FpOps> *row = table + (size_t)i * windows * entries;
#pragma unroll 1
    for (u32 win = 0; win < windows; win++) {
      const u32 d = (k.l[(win * w) >> 5] >> ((win * w) & 31)) & entries;
      if (!d) continue;
      const Affine<FpOps> e = row[(size_t)win * entries + d - 1];
      if (!aff_is_identity(e)) xyzz_madd(acc, e);
    }
  }
  const Affine<FpOps> first = *ic0;
  if (!aff_is_identity(first)) xyzz_madd(acc, first);
  Affine<FpOps> r;
  xyzz_to_affine(r, acc);
  out[j] = r;
}
// 8. The three Miller loops of one proof: f(A_j, B_j), f(acc_j, -gamma), f(C_j, -delta).  B_j's lines are the lane's own
// (g2_lines_kernel); the key's lines (klines: -gamma's 68, then -delta's) have the same address in every lane.  The G1
// points are read again at every product instead of living in registers through the loop.  A pair with an identity on
// either side takes no part, as in miller_kernel.  Two forms, selected by the grid:
//   gridDim.y = 3 (shipped)  block row y runs pair y alone and writes f[y n + j]: 3 n lanes, then two products per proof
//                            (f12_fold_kernel).  15.7 k Fp products per proof.
//   gridDim.y = 1            one lane per proof multiplies the pairs of `pairs` (7: all) under ONE chain of squarings,
//                            the reference's multi_miller_loop: one Fp12 squaring and three sparse line products per
//                            step, 11.0 k Fp products per proof.
// A 2^14-proof chunk is 256 waves on 1024 SIMDs at one wave per SIMD, so a launch costs one wave's latency and not the
// chip's throughput: the shared form's lane does twice the work of a one-pair lane and takes twice as long (16.6 against
// 8.2 + 0.2 ms per chunk, profiles/verify_each_bench.json), while the three-loop form's 768 waves still fit the chip at
// once.  The shared form is kept behind BELLMAN_HIP_VERIFY_EACH_SHARED=1 for tools/bench_verify_each.py.
__global__ __launch_bounds__(64) void miller3_kernel(const Affine<FpOps> *a, const Affine<FpOps> *acc, const ProofRec *proofs,
                                                     const line_t *blines, const u32 *bflags, const line_t *__restrict__ klines,
                                                     const u32 *__restrict__ kflags, u32 pairs, fp12_t *f, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (gridDim.y > 1) {
    pairs = 1u << blockIdx.y;
    f += (size_t)blockIdx.y * n;
  }
  const Affine<FpOps> *pa = a + i, *pg = acc + i, *pc = &proofs[i].c;
  const line_t *bl = blines + (size_t)i * MILLER_LINES;
  const bool on0 = (pairs & 1u) && !aff_is_identity(*pa) && !(bflags[i] & PF_IDENTITY);
  const bool on1 = (pairs & 2u) && !aff_is_identity(*pg) && !(kflags[0] & PF_IDENTITY);
  const bool on2 = (pairs & 4u) && !aff_is_identity(*pc) && !(kflags[1] & PF_IDENTITY);
  fp12_t r;
  f12_one(r);
  int k = 0;
#pragma unroll 1
  for (int s = 62; s >= 0; s--) {
    if (s != 62) f12_sqr(r, r);   // r = 1 before the first step
    const int steps = ((BLS_X_ABS >> s) & 1) ? 2 : 1;
#pragma unroll 1
    for (int t = 0; t < steps; t++, k++) {
      if (on0) f12_mul_line_at(r, bl[k], pa->x, pa->y);
      if (on1) f12_mul_line_at(r, klines[k], pg->x, pg->y);
      if (on2) f12_mul_line_at(r, klines[MILLER_LINES + k], pc->x, pc->y);
    }
  }
  f[i] = r;
}
// f[i] *= *c: the key's constant f(-alpha, beta) into every proof's product
__global__ __launch_bounds__(64) void f12_mul_const_kernel(fp12_t *f, const fp12_t *c, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12_t x = f[i], y = *c;
  f12_mul(x, x, y);
  f[i] = x;
}
// 9. the code bh_groth16_verify returns for proof j alone - after, for proofs given as bytes, the code bh_proofs_read
// returns for it (words: its status words, or NULL): a read error, else a point off its curve, else the pairing check
__global__ __launch_bounds__(256) void verdict_kernel(const u32 *words, const u32 *pflags, const u32 *qflags, const u32 *is_one,
                                                      int *verdicts, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int v = BH_OK;
  if (words)
    for (int k = 0; k < 3 && v == BH_OK; k++) {   // proof_status_error: the first bad element in the order a, b, c
      const u32 s = (words[i] >> (8 * k)) & 0xffu;
      if (s & PT_INVALID_MASK) v = BH_ERR_INVALID_POINT;
      else if (s & PT_IS_INF) v = BH_ERR_POINT_AT_INFINITY;
    }
  if (v == BH_OK) {
    if ((pflags[i] | qflags[i]) & PF_OFF_CURVE) v = BH_ERR_INVALID_POINT;
    else if (is_one[i] != 1u) v = BH_ERR_INVALID_PROOF;
  }
  verdicts[i] = v;
}

// ---- proofs of several keys in one call (bh_groth16_verify_each_keys, bh_groth16_batch_verify_keys) ----------------------
// The host groups the rows of a chunk by key (a stable counting sort) and cuts every key's run into blocks of at most 64
// rows, so that a 64-lane block belongs to ONE key: the block fetches its KeyBlock and the key's KeyDesc by blockIdx, and
// the key's pointers stay wave-uniform (scalar loads), as the kernel arguments of the one-key kernels are.  Rows are
// addressed in the grouped order; the host carries verdicts and status words back through the permutation.
struct KeyDesc {                // one per key of a bh_pvk_set (device table, immutable once written)
  const line_t *lines;          // [3][68]: -gamma, -delta, beta
  const u32 *qflags;            // [3]
  const Affine<FpOps> *alpha;
  const Affine<FpOps> *table;   // window table of ic_1 .. ic_n (NULL for a key without inputs), its width below
  const Affine<FpOps> *ic0;
  const fp12_t *f_ab;           // f(-alpha, beta)
  u32 w, n_inputs;
  u32 col_off, pad;             // the key's first column in the set's column sums (n_inputs + 1 columns per key)
};
struct KeyBlock {               // rows [first, first + count) of the grouped chunk belong to `key`; count <= 64;
  u32 key, first, count, in_off;   // the inputs of row first + t are the n_inputs scalars from in_off + t * n_inputs on
};
struct KeySeg {                 // a key's whole run of rows in the grouped chunk (count may be 0) and its first input
  u32 first, count, in_off, pad;
};

// 7k. ic_accumulate_kernel from the row's own key: its table, width and ic_0, the ragged input offset
__global__ __launch_bounds__(64) void ic_accumulate_keys_kernel(const fr_t *inputs, int fmt, const KeyDesc *__restrict__ keys,
                                                                const KeyBlock *__restrict__ blocks, Affine<FpOps> *out) {
  const KeyBlock b = blocks[blockIdx.x];
  if (threadIdx.x >= b.count) return;
  const KeyDesc kd = keys[b.key];
  const u32 w = kd.w, n_inputs = kd.n_inputs;
  const fr_t *in = inputs + (size_t)b.in_off + (size_t)threadIdx.x * n_inputs;
  const u32 entries = (1u << w) - 1, windows = 256 / w;
  XYZZ<FpOps> acc;
  xyzz_set_identity(acc);
#pragma unroll 1
  for (u32 i = 0; i < n_inputs; i++) {
    fr_t k;
    scalar_bits(k, in[i], fmt);
    const Affine<FpOps> *row = kd.table + (size_t)i * windows * entries;
#pragma unroll 1
    for (u32 win = 0; win < windows; win++) {
      const u32 d = (k.l[(win * w) >> 5] >> ((win * w) & 31)) & entries;
      if (!d) continue;
      const Affine<FpOps> e = row[(size_t)win * entries + d - 1];
      if (!aff_is_identity(e)) xyzz_madd(acc, e);
    }
  }
  const Affine<FpOps> first = *kd.ic0;
  if (!aff_is_identity(first)) xyzz_madd(acc, first);
  Affine<FpOps> r;
  xyzz_to_affine(r, acc);
  out[b.first + threadIdx.x] = r;
}
// 8k. miller3_kernel with the -gamma and -delta lines of the row's key, in both grid forms (n: the rows of the chunk)
__global__ __launch_bounds__(64) void miller3_keys_kernel(const Affine<FpOps> *a, const Affine<FpOps> *acc, const ProofRec *proofs,
                                                          const line_t *blines, const u32 *bflags, const KeyDesc *__restrict__ keys,
                                                          const KeyBlock *__restrict__ blocks, u32 pairs, fp12_t *f, u32 n) {
  const KeyBlock b = blocks[blockIdx.x];
  if (threadIdx.x >= b.count) return;
  const u32 i = b.first + threadIdx.x;
  const line_t *__restrict__ klines = keys[b.key].lines;
  const u32 *__restrict__ kflags = keys[b.key].qflags;
  if (gridDim.y > 1) {
    pairs = 1u << blockIdx.y;
    f += (size_t)blockIdx.y * n;
  }
  const Affine<FpOps> *pa = a + i, *pg = acc + i, *pc = &proofs[i].c;
  const line_t *bl = blines + (size_t)i * MILLER_LINES;
  const bool on0 = (pairs & 1u) && !aff_is_identity(*pa) && !(bflags[i] & PF_IDENTITY);
  const bool on1 = (pairs & 2u) && !aff_is_identity(*pg) && !(kflags[0] & PF_IDENTITY);
  const bool on2 = (pairs & 4u) && !aff_is_identity(*pc) && !(kflags[1] & PF_IDENTITY);
  fp12_t r;
  f12_one(r);
  int k = 0;
#pragma unroll 1
  for (int s = 62; s >= 0; s--) {
    if (s != 62) f12_sqr(r, r);
    const int steps = ((BLS_X_ABS >> s) & 1) ? 2 : 1;
#pragma unroll 1
    for (int t = 0; t < steps; t++, k++) {
      if (on0) f12_mul_line_at(r, bl[k], pa->x, pa->y);
      if (on1) f12_mul_line_at(r, klines[k], pg->x, pg->y);
      if (on2) f12_mul_line_at(r, klines[MILLER_LINES + k], pc->x, pc->y);
    }
  }
  f[i] = r;
}
// f[row] *= f(-alpha, beta) of the row's key
__global__ __launch_bounds__(64) void f12_mul_const_keys_kernel(fp12_t *f, const KeyDesc *__restrict__ keys,
                                                                const KeyBlock *__restrict__ blocks) {
  const KeyBlock b = blocks[blockIdx.x];
  if (threadIdx.x >= b.count) return;
  const u32 i = b.first + threadIdx.x;
  fp12_t x = f[i], y = *keys[b.key].f_ab;
  f12_mul(x, x, y);
  f[i] = x;
}
// 3k. segmented column sums: for key k = blockIdx.y / nb and its run of rows, part[(col_off_k + col) * nb + block] as
// fr_colsum_kernel writes it for one key; block columns beyond the key's n_inputs + 1 leave at once.  The columns of all
// keys lie side by side, so fr_colsum_finish_kernel over the set's total column count finishes them.
__global__ __launch_bounds__(COLSUM_THREADS) void fr_colsum_keys_kernel(const fr_t *z, const fr_t *inputs, int fmt,
                                                                        const KeyDesc *__restrict__ keys,
                                                                        const KeySeg *__restrict__ segs, u32 nb, fr_t *part) {
  __shared__ fr_t sh[COLSUM_THREADS];
  const u32 key = blockIdx.y / nb, by = blockIdx.y % nb, col = blockIdx.x, t = threadIdx.x;
  const u32 n_inputs = keys[key].n_inputs;
  if (col > n_inputs) return;
  const KeySeg s = segs[key];
  fr_t acc;
  fe_zero(acc);
  for (u32 j = by * COLSUM_THREADS + t; j < s.count; j += nb * COLSUM_THREADS) {
    fr_t zm, term;
    scalar_mont(zm, z[s.first + j], fmt);
    if (col == 0) term = zm;
    else {
      fr_t a;
      scalar_mont(a, inputs[(size_t)s.in_off + (size_t)j * n_inputs + col - 1], fmt);
      fe_mul(term, zm, a);
    }
    fe_add(acc, acc, term);
  }
  sh[t] = acc;
  __syncthreads();
  for (u32 h = COLSUM_THREADS / 2; h; h >>= 1) {
    if (t < h) {
      fr_t v;
      fe_add(v, sh[t], sh[t + h]);
      sh[t] = v;
    }
    __syncthreads();
  }
  if (t == 0) part[(size_t)(keys[key].col_off + col) * nb + by] = sh[0];
}
// [acc_Y,k] alpha_k for every key of the set, one lane per key: out[k] = [acc[col_off_k]] alpha_k (Montgomery scalar)
__global__ __launch_bounds__(64) void g1_mul_keys_kernel(Affine<FpOps> *out, const KeyDesc *__restrict__ keys, const fr_t *acc,
                                                         u32 n_keys) {
  const u32 key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= n_keys) return;
  fr_t k;
  fe_from_mont(k, acc[keys[key].col_off]);
  const Affine<FpOps> a = *keys[key].alpha;
  XYZZ<FpOps> r;
  xyzz_set_identity(r);
  if (!aff_is_identity(a))
    for (int bit = 255; bit >= 0; bit--) {
      XYZZ<FpOps> t;
      xyzz_dbl(t, r);
      r = t;
      if ((k.l[bit >> 5] >> (bit & 31)) & 1) xyzz_madd(r, a);
    }
  Affine<FpOps> o;
  xyzz_to_affine(o, r);
  out[key] = o;
}
// the 3 K key pairs of a batch over a set, one lane per pair: f[which * K + k] = f(p[which * K + k], lines `which` of
// key k) for which = 0 (-gamma), 1 (-delta), 2 (beta); an identity on either side gives 1, as in miller_kernel
__global__ __launch_bounds__(64) void miller_keys_kernel(const Affine<FpOps> *p, const KeyDesc *__restrict__ keys, u32 n_keys,
                                                         fp12_t *f) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * n_keys) return;
  const u32 which = i / n_keys, key = i % n_keys;
  const Affine<FpOps> pp = p[i];
  const line_t *l = keys[key].lines + (size_t)which * MILLER_LINES;
  const u32 qf = keys[key].qflags[which];
  fp12_t r;
  if (aff_is_identity(pp) || (qf & PF_IDENTITY)) {
    f12_one(r);
  } else {
    miller_loop_lines(r, pp.x, pp.y, [&](int k) { return l[k]; });
  }
  f[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static u32 blocks_of(size_t n, u32 t) { return (u32)((n + t - 1) / t); }

int launch_g2_lines(hipStream_t st, const void *q_dev, size_t stride_bytes, int negate, line_t *lines, u32 *flags, size_t n) {
  if (!n) return BH_OK;
  (void)hipGetLastError();   // a handled error of an earlier call on this thread is not ours
  hipLaunchKernelGGL(g2_lines_kernel, dim3(blocks_of(n, 64)), dim3(64), 0, st, (const Affine<Fp2Ops> *)q_dev, stride_bytes / 4,
                     negate, lines, flags, (u32)n);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
int launch_miller(hipStream_t st, const Affine<FpOps> *p, const line_t *lines, const u32 *qflags, fp12_t *f, size_t n,
                  const line_t *lines1, const u32 *qflags1, size_t n1) {
  if (!(n + n1)) return BH_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(miller_kernel, dim3(blocks_of(n + n1, 64)), dim3(64), 0, st, p, lines, qflags, (u32)n, lines1, qflags1, f,
                     (u32)(n + n1));
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// product of f[0..m) into f[0]
int launch_fold(hipStream_t st, fp12_t *f, size_t m) {
  while (m > 1) {
    const size_t h = (m + 1) / 2;
    (void)hipGetLastError();
    hipLaunchKernelGGL(f12_fold_kernel, dim3(blocks_of(m - h, 64)), dim3(64), 0, st, f, (u32)m, (u32)h);
    BH_HIP_CHECK(hipGetLastError());
    m = h;
  }
  return BH_OK;
}
// m products of two factors each, laid out as two rows: f[i] *= f[m + i] for i < m (one launch)
int launch_fold_rows(hipStream_t st, fp12_t *f, size_t m) {
  if (!m) return BH_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(f12_fold_kernel, dim3(blocks_of(m, 64)), dim3(64), 0, st, f, (u32)(2 * m), (u32)m);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// f^(3 (p^12 - 1) / q) (canonical) and its test against 1, for n values; ws: 4 n Fp12
int launch_final_exp(hipStream_t st, const fp12_t *f, size_t n, fp12_t *out, u32 *is_one, fp12_t *ws) {
  if (!final_exp_chain(st, f, out, is_one, ws, (u32)n)) {
    fprintf(stderr, "[bellman_hip] final exponentiation: launch failed\n");
    return BH_ERR_HIP;
  }
  return BH_OK;
}

// the column sums of one chunk: part[col * nb + block] by fr_colsum_kernel, then acc[col] += the column's nb partial sums
// (part: ncol * COLSUM_BLOCKS values).  nb = 0: one block row per COLSUM_THREADS proofs, COLSUM_BLOCKS at the most - what
// the batch verifier runs; any other nb <= COLSUM_BLOCKS is for the stage tests (tests/test_gpu_pairing_stages.py)
static int launch_colsum(hipStream_t st, const fr_t *z, const fr_t *inputs, size_t n_inputs, int fmt, size_t m, fr_t *part, fr_t *acc,
                         u32 nb = 0) {
  const size_t ncol = n_inputs + 1;
  if (!nb) nb = (u32)std::min<size_t>(COLSUM_BLOCKS, blocks_of(m, COLSUM_THREADS));
  (void)hipGetLastError();
  hipLaunchKernelGGL(fr_colsum_kernel, dim3((u32)ncol, nb), dim3(COLSUM_THREADS), 0, st, z, inputs, (u32)n_inputs, fmt, (u32)m, part);
  hipLaunchKernelGGL(fr_colsum_finish_kernel, dim3(blocks_of(ncol, 64)), dim3(64), 0, st, part, nb, (u32)ncol, acc);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// per proof, after miller3_kernel: f[j] *= f[m + j] * f[2 m + j] where the three pairs ran apart (separate), then f[j] *= *c
static int launch_fold3_const(hipStream_t st, fp12_t *f, const fp12_t *c, size_t m, bool separate) {
  if (!m) return BH_OK;
  const dim3 g(blocks_of(m, 64)), blk(64);
  (void)hipGetLastError();
  if (separate) {
    hipLaunchKernelGGL(f12_fold_kernel, g, blk, 0, st, f + m, (u32)(2 * m), (u32)m);
    hipLaunchKernelGGL(f12_fold_kernel, g, blk, 0, st, f, (u32)(2 * m), (u32)m);
  }
  hipLaunchKernelGGL(f12_mul_const_kernel, g, blk, 0, st, f, c, (u32)m);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// ---- several keys: `blocks` holds nblocks KeyBlock of the grouped chunk, `keys` the set's descriptors (both on the device)
static int launch_ic_accumulate_keys(hipStream_t st, const fr_t *inputs, int fmt, const KeyDesc *keys, const KeyBlock *blocks,
                                     size_t nblocks, Affine<FpOps> *out) {
  if (!nblocks) return BH_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(ic_accumulate_keys_kernel, dim3((u32)nblocks), dim3(64), 0, st, inputs, fmt, keys, blocks, out);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// f: 3 m values where the three pairs run apart (separate), else m
static int launch_miller3_keys(hipStream_t st, const Affine<FpOps> *a, const Affine<FpOps> *acc, const ProofRec *proofs,
                               const line_t *blines, const u32 *bflags, const KeyDesc *keys, const KeyBlock *blocks, size_t nblocks,
                               bool separate, fp12_t *f, size_t m) {
  if (!nblocks) return BH_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(miller3_keys_kernel, dim3((u32)nblocks, separate ? 3 : 1), dim3(64), 0, st, a, acc, proofs, blines, bflags,
                     keys, blocks, 7u, f, (u32)m);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// launch_fold3_const with the constant of every row's key
static int launch_fold3_const_keys(hipStream_t st, fp12_t *f, const KeyDesc *keys, const KeyBlock *blocks, size_t nblocks, size_t m,
                                   bool separate) {
  if (!m || !nblocks) return BH_OK;
  const dim3 g(blocks_of(m, 64)), blk(64);
  (void)hipGetLastError();
  if (separate) {
    hipLaunchKernelGGL(f12_fold_kernel, g, blk, 0, st, f + m, (u32)(2 * m), (u32)m);
    hipLaunchKernelGGL(f12_fold_kernel, g, blk, 0, st, f, (u32)(2 * m), (u32)m);
  }
  hipLaunchKernelGGL(f12_mul_const_keys_kernel, dim3((u32)nblocks), blk, 0, st, f, keys, blocks);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// the column sums of one grouped chunk for every key of the set: one launch whatever n_keys is, then the finish step over
// the set's total_cols columns (part: total_cols * COLSUM_BLOCKS values; acc: total_cols).  max_seg: the longest run of
// the chunk; max_cols: the largest n_inputs + 1 of the set; nb as for launch_colsum
static int launch_colsum_keys(hipStream_t st, const fr_t *z, const fr_t *inputs, int fmt, const KeyDesc *keys, const KeySeg *segs,
                              size_t n_keys, size_t max_cols, size_t total_cols, size_t max_seg, fr_t *part, fr_t *acc, u32 nb = 0) {
  if (!nb) nb = (u32)std::max<size_t>(1, std::min<size_t>(COLSUM_BLOCKS, blocks_of(max_seg, COLSUM_THREADS)));
  (void)hipGetLastError();
  hipLaunchKernelGGL(fr_colsum_keys_kernel, dim3((u32)max_cols, (u32)(n_keys * nb)), dim3(COLSUM_THREADS), 0, st, z, inputs, fmt,
                     keys, segs, nb, part);
  hipLaunchKernelGGL(fr_colsum_finish_kernel, dim3(blocks_of(total_cols, 64)), dim3(64), 0, st, part, nb, (u32)total_cols, acc);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
static int launch_g1_mul_keys(hipStream_t st, Affine<FpOps> *out, const KeyDesc *keys, const fr_t *acc, size_t n_keys) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(g1_mul_keys_kernel, dim3(blocks_of(n_keys, 64)), dim3(64), 0, st, out, keys, acc, (u32)n_keys);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// p, f: 3 n_keys values, [which][key]
static int launch_miller_keys(hipStream_t st, const Affine<FpOps> *p, const KeyDesc *keys, size_t n_keys, fp12_t *f) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(miller_keys_kernel, dim3(blocks_of(3 * n_keys, 64)), dim3(64), 0, st, p, keys, (u32)n_keys, f);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // namespace bh
