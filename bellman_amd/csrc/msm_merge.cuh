// Stage 4 of a multiexp, second half: the kernels that fold the partial sums of buckets that straddle chunk boundaries
// (planned by merge_plan of msm_stage_plans.hpp, launched by launch_merges of msm_ec.cuh).
#pragma once
#include <type_traits>

#include "msm_accumulate.cuh"
#include "msm_sums.cuh"

namespace bh {

// Last chunk that holds a head partial of the run with digit d, given that the run continues from chunk `lane`
// into chunk lane + 1: the last chunk whose FIRST entry has digit d.  Galloping + binary search over the chunk
// starts (8-byte probes of the sorted stream): one or two probes for the usual two-chunk run.
__device__ __forceinline__ u32 run_last_chunk(const u64 *src, u32 n, u32 z, u32 K, u32 lane, u32 d) {
  const u32 nchunks = (u32)(((u64)(n - z) + K - 1) / K);
  u32 lo = lane + 1, step = 1, hi;
  for (;;) {
    hi = lo + step;
    if (hi >= nchunks) { hi = nchunks; break; }
    if ((u32)(src[(u64)z + (u64)hi * K] >> 32) != d) break;
    lo = hi;
    step <<= 1;
  }
  while (hi - lo > 1) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if ((u32)(src[(u64)z + (u64)mid * K] >> 32) == d) lo = mid; else hi = mid;
  }
  return lo;
}

// Folds the partial sums of buckets that straddle chunk boundaries.  The lane whose chunk holds the run's first
// entry owns it: it finds the run's last chunk, folds tail[l0] + head[l0+1 .. l1] itself when that is at most
// `walk` additions, and queues longer runs - medium ones for the G-workers-per-run part of msm_merge_tail_kernel, runs of
// more than `big_chunks` chunks cut into workgroup-sized pieces for its long part - so that no lane ever executes a long
// serial chain of point additions (~20 us per link).
// wavefronts per SIMD the register allocation aims at (hipcc reads the second launch bound that way): two for every
// bundle whose lane state allows it - the lane-triple instantiation sat at 256 VGPRs + 2 AGPRs, one wavefront per SIMD
// for two registers (profiles/archive/r4_call8.txt: G2 reduce 1.0 -> 0.91-0.94 ms)
template <class F>
constexpr int merge_waves_per_simd() { return (F::LANES == 1 && F::WORDS == 24) ? 1 : 2; }
template <class F>
__global__ __launch_bounds__(128, merge_waves_per_simd<F>()) void msm_merge_chunks_kernel(const u64 *pairs, const u32 *zstart,
                                                               XYZZ<typename F::Mem> *pts,
                                                               const XYZZ<typename F::Mem> *head,
                                                               const XYZZ<typename F::Mem> *tail, u32 n, u32 c, u32 K,
                                                               u32 chunks_per_window, u32 walk, LongRun *long_runs,
                                                               u32 max_long, BigRun *big_runs, u32 max_big, u32 big_chunks,
                                                               u32 piece, ErrFlags *err) {
  const u32 w = blockIdx.y;
  u32 in_block, lane;
  if (!worker_index<F>(default_per_wave<F>(), in_block, lane)) return;
  const u64 *src = pairs + (u64)w * n;
  const u32 z = zstart[w];
  K = effective_chunk(n, z, chunks_per_window, K);   // the same rule as the accumulation
  ChunkView v;
  if (lane >= chunks_per_window || !chunk_view(src, n, z, lane, K, v)) return;
  if (!v.tail_partial) return;
  if (v.head_partial && v.d_first == v.d_last) return;   // a middle piece of a long bucket
  const u32 d = v.d_last;
  const u32 last = run_last_chunk(src, n, z, K, lane, d);
  if (last - lane > walk) {
    if (worker_role<F>() == 0) {   // one entry per worker
      if (last - lane > big_chunks) {   // cut into workgroup-sized pieces (msm_merge_tail_kernel, long part)
        const u32 slot = atomicAdd(&err->nbig, 1u);
        const u32 np = (last - lane + piece) / piece;   // ceil(partials / piece), partials = last - lane + 1
        const u32 p0 = atomicAdd(&err->npieces, np);
        if (slot < max_big) { BigRun br = {w, lane, d, last, p0, np, 0u, 0u}; big_runs[slot] = br; }
      } else {
        const u32 slot = atomicAdd(&err->nlong, 1u);
        if (slot < max_long) { LongRun lr = {w, lane, d, last}; long_runs[slot] = lr; }
      }
    }
    return;
  }
  const u64 slot0 = (u64)w * chunks_per_window;
  XYZZ<F> acc;
  load_xyzz<F>(acc, tail + slot0 + lane);
  for (u32 j = lane + 1; j <= last; j++) {
    XYZZ<F> o, r;
    load_xyzz<F>(o, head + slot0 + j);
    xyzz_add(r, acc, o);
    acc = r;
  }
  store_xyzz<F>(&pts[((u64)w << (c - 1)) + d - 1], acc);
}

// ============================================================================================
// 4''. very long bucket runs: workgroup-sized pieces, the last workgroup to finish folds the piece results
// ============================================================================================
// What a run of L partials costs is the DEPTH of its addition tree times the latency of a point addition (~19 us on a
// wavefront that has its SIMD to itself, ~10 us on lane pairs), not the number of additions: round 5 gave every such run
// ONE workgroup of 512 workers - ceil(L / 512) serial additions + 9 tree levels at two wavefronts per SIMD (37 us a level):
// 0.59 ms for the 5 461 partials of bucket 1 of a 50 %-boolean 2^20-term multiexp, 7.5 ms for an all-ones vector over a
// window table, 4.2 ms for a 90 %-boolean G2 query of 2^19 points (profiles/r6_call2_boolean_kernels.txt).  Now a run is cut
// into pieces of 2 x (workers of a 256-thread workgroup) partials - one serial addition, then the tree, four wavefronts on
// four SIMDs - spread over the chip, and the workgroup that finishes a run's last piece (a counter in the run's record)
// folds the piece results the same way: depth ~ log2 L + 2.
// sum over the workgroup's workers -> worker 0 (every thread of the workgroup calls it)
template <class WK>
__device__ __forceinline__ void long_block_sum(typename WK::Pt &acc, bool live, u32 wid, typename WK::Pt (*wave_part)[WK::LANES]) {
  fold_over_waves<WK>(acc, live, WK::PER_WAVE, LONG_THREADS / 64, wid, wave_part);
  __syncthreads();
}
// Medium runs: tail[l0] + sum of head[l0+1 .. l1] by G workers per run (G a power of two chosen by the host, PER_WAVE / G
// runs per wavefront): every worker folds every G-th partial, then a shuffle tree.  The case this is for: the top window
// of the 13-bit plans and the buckets of window-table plans, a few times fuller than a chunk (8-32 chunks).  Wavefront
// `wave` of `nwaves` (no barrier in here: the wavefronts of a workgroup proceed independently).
template <class WK>
__device__ __forceinline__ void merge_medium_runs(XYZZ<typename WK::Mem> *pts, const XYZZ<typename WK::Mem> *head,
                                                  const XYZZ<typename WK::Mem> *tail, u32 c, u32 chunks_per_window,
                                                  const LongRun *runs, u32 nruns, u32 G, u32 wave, u32 nwaves) {
  typedef typename WK::Pt Pt;
  constexpr u32 PW = WK::PER_WAVE;
  u32 wid;
  const bool live = WK::index(wid);
  const u32 t = wid - (threadIdx.x >> 6) * PW;   // worker inside the wavefront
  const u32 per_wave = PW / G, r = t / G, k = t & (G - 1);
  for (u32 base = wave * per_wave; base < nruns; base += nwaves * per_wave) {
    const u32 e = base + r;
    const bool valid = live && e < nruns;
    LongRun lr = {0, 0, 0, 0};
    if (valid) lr = runs[e];
    const u64 slot0 = (u64)lr.w * chunks_per_window;
    Pt acc;
    WK::identity(acc);
    if (valid) {
      if (k == 0) WK::load(acc, tail + slot0 + lr.lane);
      for (u32 j = lr.lane + 1 + k; j <= lr.last; j += G) {
        Pt o;
        WK::load(o, head + slot0 + j);
        WK::add(acc, o);
      }
    }
    WK::tree(acc, G, k);   // (every lane of the wavefront takes part in the shuffles)
    if (valid && k == 0) WK::store(&pts[((u64)lr.w << (c - 1)) + lr.d - 1], acc);
  }
}
// Big runs, piece by piece: workgroup `blk` of `nblk`.
template <class WK>
__device__ __forceinline__ void merge_big_runs(XYZZ<typename WK::Mem> *pts, const XYZZ<typename WK::Mem> *head,
                                               const XYZZ<typename WK::Mem> *tail, u32 c, u32 chunks_per_window,
                                               BigRun *runs, u32 nruns, XYZZ<typename WK::Mem> *piece_out, u32 total,
                                               u32 blk, u32 nblk, void *lds_part, u32 *sh_run, u32 *sh_last) {
  typedef typename WK::Pt Pt;
  constexpr u32 NWORK = long_workers<WK>(), PIECE = long_piece<WK>();
  Pt(*wave_part)[WK::LANES] = reinterpret_cast<Pt(*)[WK::LANES]>(lds_part);
  u32 wid;
  const bool live = WK::index(wid);   // idle lanes stay for the barriers
  for (u32 piece = blk; piece < total; piece += nblk) {
    if (threadIdx.x == 0) *sh_run = 0xffffffffu;
    __syncthreads();
    for (u32 e = threadIdx.x; e < nruns; e += LONG_THREADS)
      if (piece - runs[e].piece0 < runs[e].npieces) *sh_run = e;   // exactly one run owns the piece
    __syncthreads();
    const u32 e = *sh_run;
    if (e == 0xffffffffu) continue;   // (uniform over the workgroup)
    const u32 rw = runs[e].w, rlane = runs[e].lane, rd = runs[e].d, rlast = runs[e].last, p0 = runs[e].piece0, np = runs[e].npieces;
    const u64 slot0 = (u64)rw * chunks_per_window;
    XYZZ<typename WK::Mem> *out = &pts[((u64)rw << (c - 1)) + rd - 1];
    // partial t of the run: t == 0 the tail partial of its first chunk, then the head partials of the chunks that follow
    const u32 t0 = (piece - p0) * PIECE, nparts = rlast - rlane + 1;
    const u32 t1 = t0 + PIECE < nparts ? t0 + PIECE : nparts;
    Pt acc;
    WK::identity(acc);
    if (live)
      for (u32 t = t0 + wid; t < t1; t += NWORK) {
        Pt o;
        WK::load(o, t == 0 ? tail + slot0 + rlane : head + slot0 + rlane + t);
        WK::add(acc, o);
      }
    long_block_sum<WK>(acc, live, wid, wave_part);
    if (np == 1) {
      if (live && wid == 0) WK::store(out, acc);
      continue;
    }
    if (live && wid == 0) WK::store(&piece_out[piece], acc);
    __threadfence();   // the piece result is visible device-wide before the counter moves
    __syncthreads();
    if (threadIdx.x == 0) *sh_last = atomicAdd(&runs[e].done, 1u) == np - 1 ? 1u : 0u;
    __syncthreads();
    if (*sh_last) {   // every other piece of the run has been published: fold them
      __threadfence();
      WK::identity(acc);
      if (live)
        for (u32 q = wid; q < np; q += NWORK) {
          Pt o;
          WK::load(o, &piece_out[p0 + q]);
          WK::add(acc, o);
        }
      long_block_sum<WK>(acc, live, wid, wave_part);
      if (live && wid == 0) WK::store(out, acc);
    }
  }
}
// The two parts as launches of their own (one wavefront per workgroup for the medium runs): what the tiny G2 tables run.
// The fused kernel below needs 256-thread workgroups for its long part, and the lane-triple instantiation then allocates
// 256 VGPRs + 47 AGPRs where this one fits 256 + 0 - the medium runs of a window table over 2^10 G2 points (128 runs of
// 32 partials, the whole job) took 351 us fused against ~230 us here (profiles/r6_call14_small_jobs.txt,
// r6_call15_tail_split_ab.txt).
template <class WK>
__global__ __launch_bounds__(64, WK::LANES == 1 && sizeof(typename WK::Pt) > 200 ? 1 : 2) void msm_merge_runs_kernel(
    XYZZ<typename WK::Mem> *pts, const XYZZ<typename WK::Mem> *head, const XYZZ<typename WK::Mem> *tail, u32 c,
    u32 chunks_per_window, const LongRun *runs, u32 max_runs, u32 G, const ErrFlags *err) {
  u32 nruns = err->nlong;
  if (nruns > max_runs) nruns = max_runs;
  merge_medium_runs<WK>(pts, head, tail, c, chunks_per_window, runs, nruns, G, blockIdx.x, gridDim.x);
}
template <class WK>
__global__ __launch_bounds__(LONG_THREADS) void msm_merge_long_kernel(XYZZ<typename WK::Mem> *pts,
                                                                      const XYZZ<typename WK::Mem> *head,
                                                                      const XYZZ<typename WK::Mem> *tail, u32 c,
                                                                      u32 chunks_per_window, BigRun *big_runs, u32 max_big,
                                                                      XYZZ<typename WK::Mem> *piece_out, u32 max_pieces,
                                                                      const ErrFlags *err) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_part[sizeof(typename WK::Pt) * (LONG_THREADS / 64) * WK::LANES];
  __shared__ u32 sh_run, sh_last;
  u32 nbig = err->nbig, total = err->npieces;
  if (nbig > max_big) nbig = max_big;
  if (total > max_pieces) total = max_pieces;
  merge_big_runs<WK>(pts, head, tail, c, chunks_per_window, big_runs, nbig, piece_out, total, blockIdx.x, gridDim.x, lds_part,
                     &sh_run, &sh_last);
}
// ONE launch for both: workgroups [0, run_blocks) fold the medium runs (a wavefront each at a time, worker policy WKR),
// the rest the pieces of the big runs (policy WKL) - side by side, not one after the other: a window table over 2^16
// points has 4 096 medium runs AND ~115 big ones (the top row's 8-bit digits), 130 us + 170 us as two launches
// (profiles/r6_call7_k2_ab.txt).
template <class WKR, class WKL>
__global__ __launch_bounds__(LONG_THREADS) void msm_merge_tail_kernel(XYZZ<typename WKL::Mem> *pts,
                                                                      const XYZZ<typename WKL::Mem> *head,
                                                                      const XYZZ<typename WKL::Mem> *tail, u32 c,
                                                                      u32 chunks_per_window, const LongRun *runs, u32 max_runs,
                                                                      u32 G, u32 run_blocks, BigRun *big_runs, u32 max_big,
                                                                      XYZZ<typename WKL::Mem> *piece_out, u32 max_pieces,
                                                                      const ErrFlags *err) {
  static_assert(std::is_same<typename WKR::Mem, typename WKL::Mem>::value, "both parts work on the same records");
  __shared__ __attribute__((aligned(16))) unsigned char lds_part[sizeof(typename WKL::Pt) * (LONG_THREADS / 64) * WKL::LANES];
  __shared__ u32 sh_run, sh_last;
  if (blockIdx.x < run_blocks) {
    u32 nruns = err->nlong;
    if (nruns > max_runs) nruns = max_runs;   // (cannot happen: max_long is an upper bound, msm_enqueue)
    merge_medium_runs<WKR>(pts, head, tail, c, chunks_per_window, runs, nruns, G,
                           blockIdx.x * (LONG_THREADS / 64) + (threadIdx.x >> 6), run_blocks * (LONG_THREADS / 64));
  } else {
    u32 nbig = err->nbig, total = err->npieces;
    if (nbig > max_big) nbig = max_big;
    if (total > max_pieces) total = max_pieces;
    merge_big_runs<WKL>(pts, head, tail, c, chunks_per_window, big_runs, nbig, piece_out, total, blockIdx.x - run_blocks,
                        gridDim.x - run_blocks, lds_part, &sh_run, &sh_last);
  }
}

}  // namespace bh
