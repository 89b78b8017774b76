// The random linear combinations of the powers-of-tau check (bh_powers_of_tau_verify, ceremony.hip): the coefficients
// expanded from a 32-byte seed on the device, and the eight sums
//   P(V) = sum_{i < n-1} rho_i V[i]      Q(V) = sum_{i < n-1} rho_i V[i + 1]
// of the four vectors as ordinary multiexps over the C ABI.  Included by ceremony.hip (the product) and by
// test_ceremony_hooks.hip (the test library), which runs both pieces on their own: tests/test_gpu_ptau_verify.py.
//
// Coefficients: block j of vector v is BLAKE2s-256 (RFC 7693), keyed with the seed, over the 24-byte message
//   "bh-ptau-rlc\0" | v as little-endian u32 | j as little-endian u64
// Coefficient 2j is bytes 0..15 of the digest read little-endian, coefficient 2j + 1 bytes 16..31; each is written as a
// 32-byte canonical little-endian scalar with the upper half zero (BH_SCALARS_CANONICAL).  128-bit coefficients: a false
// relation survives one combination with probability 2^-128.  The compression function is BH_HD, so the host build (the
// test library's bh_test_ptau_rlc_host) runs the same text without a GPU; Python's hashlib.blake2s is the reference.
#pragma once
#include <string.h>

#include "common.hpp"

namespace bh {

struct Blake2s {
  BH_HD static constexpr u32 iv(int i) {
    constexpr u32 v[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    return v[i];
  }
  BH_HD static constexpr int sigma(int r, int i) {
    constexpr unsigned char s[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    return s[r][i];
  }
};
BH_HD u32 blake2s_rotr(u32 x, int k) { return (x >> k) | (x << (32 - k)); }
#define BH_B2S_G(a, b, c, d, x, y)    \
  do {                                \
    a = a + b + (x);                  \
    d = blake2s_rotr(d ^ a, 16);      \
    c = c + d;                        \
    b = blake2s_rotr(b ^ c, 12);      \
    a = a + b + (y);                  \
    d = blake2s_rotr(d ^ a, 8);       \
    c = c + d;                        \
    b = blake2s_rotr(b ^ c, 7);       \
  } while (0)
// h <- F(h, m, t, last): one 64-byte block m (16 little-endian words), t = bytes hashed so far including this block
BH_HD void blake2s_compress(u32 h[8], const u32 m[16], u32 t, bool last) {
  u32 v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[8 + i] = Blake2s::iv(i);
  }
  v[12] ^= t;   // (t < 2^32: the high counter word stays 0)
  if (last) v[14] = ~v[14];
#pragma unroll
  for (int r = 0; r < 10; r++) {
    BH_B2S_G(v[0], v[4], v[8], v[12], m[Blake2s::sigma(r, 0)], m[Blake2s::sigma(r, 1)]);
    BH_B2S_G(v[1], v[5], v[9], v[13], m[Blake2s::sigma(r, 2)], m[Blake2s::sigma(r, 3)]);
    BH_B2S_G(v[2], v[6], v[10], v[14], m[Blake2s::sigma(r, 4)], m[Blake2s::sigma(r, 5)]);
    BH_B2S_G(v[3], v[7], v[11], v[15], m[Blake2s::sigma(r, 6)], m[Blake2s::sigma(r, 7)]);
    BH_B2S_G(v[0], v[5], v[10], v[15], m[Blake2s::sigma(r, 8)], m[Blake2s::sigma(r, 9)]);
    BH_B2S_G(v[1], v[6], v[11], v[12], m[Blake2s::sigma(r, 10)], m[Blake2s::sigma(r, 11)]);
    BH_B2S_G(v[2], v[7], v[8], v[13], m[Blake2s::sigma(r, 12)], m[Blake2s::sigma(r, 13)]);
    BH_B2S_G(v[3], v[4], v[9], v[14], m[Blake2s::sigma(r, 14)], m[Blake2s::sigma(r, 15)]);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}
#undef BH_B2S_G
// The state after the key block (the same for every block of every vector): parameter block digest 32, key 32, then the
// seed padded to 64 bytes as the first block.
BH_HD void ptau_rlc_keyed_state(u32 h[8], const u32 seed[8]) {
  u32 m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    h[i] = Blake2s::iv(i);
    m[i] = seed[i];
    m[8 + i] = 0;
  }
  h[0] ^= 0x01012020u;
  blake2s_compress(h, m, 64, false);
}
// digest of block j of vector v from the keyed state
BH_HD void ptau_rlc_block(u32 digest[8], const u32 keyed[8], u32 v, u64 j) {
  u32 m[16];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = 0;
  m[0] = 0x702d6862u;   // "bh-p"
  m[1] = 0x2d756174u;   // "tau-"
  m[2] = 0x00636c72u;   // "rlc\0"
  m[3] = v;
  m[4] = (u32)j;
  m[5] = (u32)(j >> 32);
#pragma unroll
  for (int i = 0; i < 8; i++) digest[i] = keyed[i];
  blake2s_compress(digest, m, 64 + 24, true);
}
// coefficients 2j and 2j + 1 of `count` as canonical scalars (an odd count drops the second half of the last block)
BH_HD void ptau_rlc_store(u32 *out, const u32 digest[8], u64 j, u64 count) {
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const u64 k = 2 * j + half;
    if (k >= count) return;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      out[8 * k + w] = digest[4 * half + w];
      out[8 * k + 4 + w] = 0;
    }
  }
}
struct PtauKeyed {
  u32 h[8];
};
// one lane per block (internal linkage: the test library includes this header from two units)
static __global__ __launch_bounds__(256) void ptau_rlc_kernel(PtauKeyed keyed, u32 v, u64 count, u32 *out) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (2 * j >= count) return;
  u32 d[8];
  ptau_rlc_block(d, keyed.h, v, j);
  ptau_rlc_store(out, d, j, count);
}
static inline void ptau_rlc_host(const void *seed32, u32 v, u64 count, void *out) {
  u32 seed[8], keyed[8], d[8];
  memcpy(seed, seed32, 32);
  ptau_rlc_keyed_state(keyed, seed);
  for (u64 j = 0; 2 * j < count; j++) {
    ptau_rlc_block(d, keyed, v, j);
    ptau_rlc_store((u32 *)out, d, j, count);
  }
}
// out_dev: count x 32 bytes
static inline int ptau_rlc_expand(hipStream_t st, const void *seed32, u32 v, u64 count, void *out_dev) {
  if (!count) return BH_OK;
  u32 seed[8];
  PtauKeyed keyed;
  memcpy(seed, seed32, 32);
  ptau_rlc_keyed_state(keyed.h, seed);
  const u64 blocks = (count + 1) / 2;
  (void)hipGetLastError();
  hipLaunchKernelGGL(ptau_rlc_kernel, dim3((u32)((blocks + 255) / 256)), dim3(256), 0, st, keyed, v, count, (u32 *)out_dev);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// The eight sums of a transcript: vec = tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (n_v points each); out[2 v] = P(V_v),
// out[2 v + 1] = Q(V_v) as affine records (192 bytes reserved each), rcs[...] the code of each multiexp (BH_OK,
// BH_ERR_UNEXPECTED_IDENTITY when a record it consumed is the identity); a vector of one point has empty sums: identity
// records, BH_OK.  The coefficients of all four vectors are expanded on `st`, the eight multiexps are issued together as
// ordinary jobs ordered after it (default plans: a window table is used where the handle has one) and waited for.  The
// return value carries call-level failures only.
static inline int ptau_sums(bh_ctx *ctx, const bh_bases *const vec[4], const void *seed32, hipStream_t st,
                            unsigned char out[8][192], int rcs[8]) {
  void *sc[4] = {nullptr, nullptr, nullptr, nullptr};
  bh_msm_job *jobs[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = BH_OK;
  memset(out, 0, 8 * 192);
  for (int k = 0; k < 8; k++) rcs[k] = BH_OK;
  for (u32 v = 0; v < 4 && rc == BH_OK; v++) {
    const size_t terms = bh_bases_len(vec[v]) - 1;
    if (!terms) continue;
    rc = bh_dev_alloc(ctx, terms * 32, &sc[v]);
    if (rc == BH_OK) rc = ptau_rlc_expand(st, seed32, v, terms, sc[v]);
  }
  for (u32 v = 0; v < 4 && rc == BH_OK; v++) {
    const size_t terms = bh_bases_len(vec[v]) - 1;
    if (!terms) continue;
    for (size_t skip = 0; skip < 2 && rc == BH_OK; skip++)
      rc = bh_msm_async_dev_after(ctx, vec[v], skip, sc[v], terms, BH_SCALARS_CANONICAL, nullptr, 0, nullptr, (void *)st,
                                  &jobs[2 * v + skip]);
  }
  for (int k = 0; k < 8; k++)   // every job issued is waited for, whatever happened to the others
    if (jobs[k]) {
      rcs[k] = bh_msm_wait(jobs[k], out[k]);
      if (rcs[k] != BH_OK && rcs[k] != BH_ERR_UNEXPECTED_IDENTITY && rc == BH_OK) rc = rcs[k];
    }
  if (hipStreamSynchronize(st) != hipSuccess && rc == BH_OK) rc = BH_ERR_HIP;
  for (int v = 0; v < 4; v++)
    if (sc[v]) bh_dev_free(ctx, sc[v]);
  return rc;
}

}  // namespace bh
