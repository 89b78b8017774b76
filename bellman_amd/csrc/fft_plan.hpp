// Host-only launch plans of the Fr transforms (fft.hip): how log_n splits into passes, the tile geometry of a pass,
// and the launches of a transform over k strided vectors (bh_fft_fr_many_*).  No device code and no library state: the
// test library replays these plans without a GPU (bh_test_fft_many_plan, tests/test_fft_many_model_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define BH_PLAN_HD __host__ __device__
#else
#define BH_PLAN_HD
#endif

namespace bh {

constexpr uint32_t NTT_PLAN_LOG_TILE = 11;   // 2048 Fr per workgroup (fft.hip NTT_LOG_TILE)
constexpr uint32_t NTT_PLAN_MAX_R = 11;      // rows of a tile: sub-FFT size 2^r, r <= 11

// split log_n into 1-3 passes of <= 11 bits, as evenly as possible (largest first)
inline void plan_passes(uint32_t log_n, uint32_t *r, uint32_t *L) {
  const uint32_t l = log_n <= NTT_PLAN_MAX_R ? 1 : (log_n + NTT_PLAN_MAX_R - 1) / NTT_PLAN_MAX_R;
  *L = l;
  const uint32_t q = log_n / l, rem = log_n % l;
  for (uint32_t i = 0; i < l; i++) r[i] = q + (i < rem ? 1 : 0);
}

// the geometry fields of a pass (what tile_geo and the index arithmetic of the pass kernel read)
struct NttGeo {
  uint32_t log_n, s, r, log_c, is_last, r0, L, r1, xcd_swizzle;
};
// pass p of the plan r[0..L); s = bits consumed by the passes before it
inline NttGeo pass_geo(uint32_t log_n, const uint32_t *r, uint32_t L, uint32_t p, uint32_t s) {
  NttGeo a;
  const bool last = (p == L - 1);
  a.log_n = log_n;
  a.s = s;
  a.r = r[p];
  a.is_last = last ? 1 : 0;
  a.r0 = r[0];
  a.L = L;
  a.r1 = r[1];
  // tile columns: as many as fit 2048 elements, bounded by the extent of the column dimension
  uint32_t log_c = NTT_PLAN_LOG_TILE - r[p];
  if (L == 1) log_c = 0;
  else if (last) { if (log_c > r[0]) log_c = r[0]; }
  else { uint32_t logM = log_n - s - r[p]; if (log_c > logM) log_c = logM; }
  a.log_c = log_c;
  const uint64_t tiles = ((uint64_t)1 << log_n) >> (r[p] + log_c);
  a.xcd_swizzle = (tiles >= 64 && (tiles & 7) == 0) ? 1 : 0;
  return a;
}

// One launch of the batched pass kernel.  Vectors [first_vec, first_vec + n_vec) of the call; vector j of the launch is
// read at in + j * in_stride and written at out + j * out_stride, where in / out is the caller's data (stride = the
// call's) or the scratch (stride = n, vector first_vec at scratch + 0).
//   packed (L == 1):  a tile holds 2^log_v vectors, one per column (geo.log_c == log_v); grid = ceil(n_vec / 2^log_v)
//   otherwise:        grid = tiles * n_vec; block b works on (tile, vector) = fft_many_block(...)
struct FftManyLaunch {
  uint32_t grid, threads, one_level, pass;
  uint64_t first_vec, n_vec;
  uint32_t in_scratch, out_scratch;
  uint64_t in_stride, out_stride;
  uint32_t log_v;
  NttGeo geo;
};
constexpr uint32_t FFT_MANY_MAX_GRID = 1u << 30;

// block -> (tile, vector of the launch) of a multi-pass launch.  The workgroups of one tile over the n_vec vectors are
// neighbours in issue order - on ONE XCD where the tile order is XCD-aware (blocks b, b + 8, ... share an XCD) - so a
// one-level table entry that streams from HBM for the first of them is an L2 hit for the others.
BH_PLAN_HD inline void fft_many_block(uint32_t b, uint32_t grid, uint32_t n_vec, uint32_t xcd_swizzle, uint64_t *tile, uint32_t *vec) {
  if (xcd_swizzle) {
    const uint32_t per_xcd = (grid / n_vec) >> 3, slot = b >> 3;
    *tile = (uint64_t)(b & 7u) * per_xcd + slot / n_vec;
    *vec = slot % n_vec;
  } else {
    *tile = b / n_vec;
    *vec = b % n_vec;
  }
}

// the launches of one transform of k vectors of 2^log_n (log_n < 32), `stride` elements apart, with a scratch of
// `scratch_vectors` vectors (>= 1 where log_n > 11; unused below): sub-batches of at most scratch_vectors vectors one after
// the other, every pass of a sub-batch before the next sub-batch starts
inline std::vector<FftManyLaunch> fft_many_plan(uint32_t log_n, uint64_t k, uint64_t stride, uint64_t scratch_vectors, bool one_level) {
  std::vector<FftManyLaunch> out;
  uint32_t r[3] = {0, 0, 0}, L = 1;
  plan_passes(log_n, r, &L);
  const uint64_t n = (uint64_t)1 << log_n;
  if (L == 1) {
    const uint32_t log_v = NTT_PLAN_LOG_TILE - log_n;
    uint64_t per_launch = (uint64_t)FFT_MANY_MAX_GRID << log_v;
    if (per_launch > ((uint64_t)1 << 31)) per_launch = (uint64_t)1 << 31;   // (the kernel counts a launch's vectors in 32 bits)
    for (uint64_t v0 = 0; v0 < k; v0 += per_launch) {
      FftManyLaunch l = FftManyLaunch();
      l.first_vec = v0;
      l.n_vec = k - v0 < per_launch ? k - v0 : per_launch;
      l.grid = (uint32_t)((l.n_vec + ((uint64_t)1 << log_v) - 1) >> log_v);
      l.threads = 256;   // single-pass sizes run on the two-level tables
      l.in_stride = l.out_stride = stride;
      l.log_v = log_v;
      l.geo = pass_geo(log_n, r, L, 0, 0);
      l.geo.log_c = log_v;
      out.push_back(l);
    }
    return out;
  }
  const uint64_t tiles = n >> NTT_PLAN_LOG_TILE;   // every tile of a multi-pass plan is full
  uint64_t group = scratch_vectors < 1 ? 1 : scratch_vectors;
  if (group > FFT_MANY_MAX_GRID / tiles) group = FFT_MANY_MAX_GRID / tiles;
  for (uint64_t v0 = 0; v0 < k; v0 += group) {
    uint32_t s = 0;
    for (uint32_t p = 0; p < L; p++) {
      FftManyLaunch l = FftManyLaunch();
      l.pass = p;
      l.first_vec = v0;
      l.n_vec = k - v0 < group ? k - v0 : group;
      l.grid = (uint32_t)(tiles * l.n_vec);
      l.one_level = one_level ? 1 : 0;
      l.threads = one_level ? 512 : 256;
      // ping-pong without a copy: pass 0 data -> scratch, middle passes in place in scratch, last pass scratch -> data
      l.in_scratch = p != 0;
      l.out_scratch = p != L - 1;
      l.in_stride = l.in_scratch ? n : stride;
      l.out_stride = l.out_scratch ? n : stride;
      l.geo = pass_geo(log_n, r, L, p, s);
      out.push_back(l);
      s += r[p];
    }
  }
  return out;
}

}  // namespace bh
