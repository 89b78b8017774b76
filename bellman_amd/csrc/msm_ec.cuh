// Curve-dependent part of the MSM pipeline (bucket accumulation, reductions, host tail),
// written once over the field-ops bundle and instantiated for G1 (msm_g1.hip) and G2
// (msm_g2.hip) in separate translation units so they compile in parallel.
// This file is the orchestration: the launch sequences of stages 4 and 5, msm_enqueue, msm_finish and the host tail.  A
// stage's kernels live in msm_accumulate.cuh, msm_merge.cuh and msm_sums.cuh (workers: msm_workers.cuh), its plan in
// msm_stage_plans.hpp (host only); the point kernels outside the pipeline in point_kernels.cuh.
#pragma once
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>
#include <cmath>

#include "msm_accumulate.cuh"
#include "msm_merge.cuh"
#include "msm_stage_plans.hpp"
#include "msm_sums.cuh"
#include "point_kernels.cuh"

namespace bh {

// ============================================================================================
// host side of stage 4: the two launch sequences (msm_enqueue; csrc/test_bucket_hooks.hip runs the same functions on a
// stream of the caller's choice, with the merge parameters of merge_plan)
// ============================================================================================
// 4. accumulate equal chunks ...
template <class F>
static dim3 accumulate_grid(const MsmPlan &p) {
  const u32 wpb = workers_per_block<F>(128, default_per_wave<F>());
  return dim3((p.chunks_per_window + wpb - 1) / wpb, p.W);
}
// (every variant of the kernel takes the record stride, so a padded table is read correctly by all of them)
template <class F>
static int launch_accumulate(hipStream_t st, const MsmPlan &p, bool lds_acc, const u64 *sorted, const u32 *zstart,
                             const Affine<typename F::Mem> *acc_bases, u32 acc_stride, XYZZ<typename F::Mem> *pts,
                             XYZZ<typename F::Mem> *head, XYZZ<typename F::Mem> *tail, ErrFlags *err) {
  const dim3 grid = accumulate_grid<F>(p);
  if constexpr (F::LANES == 1) {
    if (lds_acc)
      hipLaunchKernelGGL((msm_accumulate_kernel<F, true>), grid, dim3(128), 0, st, sorted, zstart, acc_bases, pts, head,
                         tail, p.n, p.c, p.chunk, p.chunks_per_window, err, acc_stride);
    else
      hipLaunchKernelGGL((msm_accumulate_kernel<F, false>), grid, dim3(128), 0, st, sorted, zstart, acc_bases, pts, head,
                         tail, p.n, p.c, p.chunk, p.chunks_per_window, err, acc_stride);
  } else {
    hipLaunchKernelGGL((msm_accumulate_kernel<F, false>), grid, dim3(128), 0, st, sorted, zstart, acc_bases, pts, head,
                       tail, p.n, p.c, p.chunk, p.chunks_per_window, err, acc_stride);
  }
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// ... then fold the buckets that straddle chunk boundaries.  block_cap (tests): 0, or at most block_cap workgroups for the
// medium runs and 2 block_cap for the pieces, so that a small job goes round the kernels' grid-stride loops
template <class FR>
static int launch_merges(hipStream_t st, const MsmPlan &p, const MergePlan &mp, int num_cus, u32 block_cap, const u64 *sorted,
                         const u32 *zstart, XYZZ<typename FR::Mem> *pts, XYZZ<typename FR::Mem> *head,
                         XYZZ<typename FR::Mem> *tail, LongRun *long_runs, BigRun *big_runs, XYZZ<typename FR::Mem> *piece_out,
                         ErrFlags *err) {
  typedef typename MergeWorkers<FR>::HalfWK HalfWK;
  constexpr bool PAIRS_POSSIBLE = MergeWorkers<FR>::PAIRS_POSSIBLE;
  const u32 max_long = mp.max_long, max_big = mp.max_big, max_pieces = mp.max_pieces, run_lanes = mp.run_lanes;
  const u32 rwpb = workers_per_block<FR>(128, default_per_wave<FR>());
  const dim3 rgrid((p.chunks_per_window + rwpb - 1) / rwpb, p.W);
  hipLaunchKernelGGL(msm_merge_chunks_kernel<FR>, rgrid, dim3(128), 0, st, sorted, zstart, pts, head, tail, p.n,
                     p.c, p.chunk, p.chunks_per_window, mp.walk, long_runs, max_long, big_runs, max_big, mp.big_chunks, mp.piece, err);
  BH_HIP_CHECK(hipGetLastError());
  // medium runs and the pieces of the big runs in ONE launch (a launch with nothing to do costs ~5 us): a wavefront per
  // SIMD for the medium runs, one workgroup per piece at a time for the big ones
  u32 run_blocks = (u32)num_cus, long_blocks = std::min<u32>(max_pieces, (u32)num_cus * 8);
  if (block_cap) { run_blocks = std::min(run_blocks, block_cap); long_blocks = std::min(long_blocks, 2 * block_cap); }
  const dim3 tgrid(run_blocks + long_blocks);
#define BH_TAIL(WKR, WKL)                                                                                                   \
  hipLaunchKernelGGL((msm_merge_tail_kernel<WKR, WKL>), tgrid, dim3(LONG_THREADS), 0, st, pts, head, tail, p.c,              \
                     p.chunks_per_window, long_runs, max_long, run_lanes, run_blocks, big_runs, max_big, piece_out,           \
                     max_pieces, err)
  // One launch (medium runs and big pieces side by side) - except the 128-bucket window tables of tiny G2 vectors, whose
  // 128 medium runs are the whole job: two launches there (G2 2^10: 0.74 against 0.85 ms; 2^12 ... 2^16 and every G1 size are
  // equal or faster fused - G1 2^16 0.79 against 0.88 ms; profiles/r6_call15_tail_split_ab.txt).  The big pieces always run
  // on the half-point worker (HalfWK is XyzzWorker<FR> where the group has none)
  if constexpr (PAIRS_POSSIBLE) {
    if (mp.runs_on_pairs) BH_TAIL(HalfWK, HalfWK);
    else BH_TAIL(XyzzWorker<FR>, HalfWK);
  } else if (p.NB > 128) {
    BH_TAIL(XyzzWorker<FR>, XyzzWorker<FR>);
  } else {
    hipLaunchKernelGGL(msm_merge_runs_kernel<XyzzWorker<FR>>, dim3(run_blocks * 4), dim3(64), 0, st, pts, head, tail, p.c,
                       p.chunks_per_window, long_runs, max_long, run_lanes, err);
    hipLaunchKernelGGL(msm_merge_long_kernel<XyzzWorker<FR>>, dim3(long_blocks), dim3(LONG_THREADS), 0, st, pts, head, tail,
                       p.c, p.chunks_per_window, big_runs, max_big, piece_out, max_pieces, err);
  }
#undef BH_TAIL
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// 4'. the one-launch small path: exactly the launch sp says (small_fill_plan over the workers per workgroup of the bundle F that
// accumulates, small_fill_workers<F>(); csrc/test_small_hooks.hip runs the same function).  pts: nb zeroed buckets;
// word_prefix (null without a density): ceil(nd / 64) + 1 words for the error-resolution pass
template <class F>
constexpr u32 small_fill_workers() { return workers_per_block<F>(SMALL_THREADS, tree_per_wave<F>()); }
template <class F>
static int launch_small_fill(hipStream_t st, const MsmPlan &p, const SmallFillPlan &sp, const void *scalars_dev, int fmt,
                             const u64 *density_dev, u32 *word_prefix, u64 skip, u64 n_bases, const Affine<typename F::Mem> *table,
                             XYZZ<typename F::Mem> *pts, ErrFlags *err) {
  if (!sp.fused || !sp.workgroups) return BH_ERR_INVALID_ARG;
  hipLaunchKernelGGL(msm_small_fill_kernel<F>, dim3(sp.workgroups), dim3(sp.threads), sp.lds_bytes, st, scalars_dev, fmt, p.nd,
                     density_dev, word_prefix, skip, n_bases, p.c, p.Wd, p.base_stride, table, pts, err);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}
// The error-resolution pass over the nd scalars of a job whose flags say both EOF and an identity (msm_finish; also run on its
// own by csrc/test_small_hooks.hip): sets err->ident_top.  bases: the records the job's accumulation read, base_stride bytes apart
template <class F>
static int launch_err_resolve(hipStream_t st, const void *scalars_dev, int fmt, u32 nd, const u64 *density_dev, const u32 *word_prefix,
                              u64 skip, u64 n_bases, const Affine<F> *bases, u32 base_stride, u32 lo_ref, ErrFlags *err) {
  hipLaunchKernelGGL(msm_err_resolve_kernel<F>, dim3((nd + 255) / 256), dim3(256), 0, st, scalars_dev, fmt, nd, density_dev,
                     word_prefix, skip, n_bases, bases, base_stride, lo_ref, err);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

// 5. reduce: the launches of rp (reduce_plan; also run on their own by csrc/test_reduce_hooks.hip), each on the sum kernel of
// its worker kind and wavefront count.  pts: NB filled buckets; rowcol, part (null unless rp.want_part), bits (zeroed): rp's
// element counts
template <class FR>
static int launch_reduce(hipStream_t st, const ReducePlan &rp, const XYZZ<typename FR::Mem> *pts, XYZZ<typename FR::Mem> *rowcol,
                         XYZZ<typename FR::Mem> *part, XYZZ<typename FR::Mem> *bits) {
  typedef typename FR::Mem M;
  XYZZ<M> *const buf[RB_BUFS] = {const_cast<XYZZ<M> *>(pts), rowcol, part, bits};   // (nothing writes RB_PTS: reduce_plan)
  if (rp.overflow) return BH_ERR_INVALID_ARG;
  for (u32 i = 0; i < rp.n_launches; i++) {
    const ReduceLaunch &l = rp.launch[i];
    SumJobs<M> js;
    for (int q = 0; q < 3; q++) {
      const ReduceJob &j = l.j[q];
      js.j[q].d = j.d; js.j[q].nblocks = j.nblocks;
      js.j[q].in = nullptr; js.j[q].out = nullptr;
      if (!j.d.groups) continue;   // nothing to do: no workgroup of the launch looks at its buffers
      if (j.in_buf >= RB_BUFS || j.out_buf >= RB_BUFS || !buf[j.in_buf] || !buf[j.out_buf]) return BH_ERR_INVALID_ARG;
      js.j[q].in = buf[j.in_buf] + j.in_off; js.j[q].out = buf[j.out_buf] + j.out_off;
    }
    const u32 kind = l.kind, waves = l.waves;
    bool known = true, ok = false;
    // (the kernels are laid out in the code object in the order they are named here)
    if constexpr (std::is_same<FR, FpOps>::value) {
      if (kind == WK_K2 && waves == 4) ok = sum_launch<K2Worker, 4>(js, st);
      else if (kind == WK_K2 && waves == 2) ok = sum_launch<K2Worker, 2>(js, st);
      else if (kind == WK_K2 && waves == 1) ok = sum_launch<K2Worker, 1>(js, st);
      else if (kind == WK_XYZZ_FP && waves == 1) ok = sum_launch<XyzzWorker<FpOps>, 1>(js, st);
      else known = false;
    } else if constexpr (std::is_same<FR, Fp2K3Ops>::value) {
      if (kind == WK_K6 && waves == 4) ok = sum_launch<K6Worker, 4>(js, st);
      else if (kind == WK_XYZZ_FP2K3 && waves == 4) ok = sum_launch<XyzzWorker<Fp2K3Ops>, 4>(js, st);
      else known = false;
    } else {
      static_assert(std::is_same<FR, Fp2Ops>::value, "the bundles that reduce: FpOps, Fp2K3Ops, Fp2Ops");
      if (kind == WK_XYZZ_FP2 && waves == 1) ok = sum_launch<XyzzWorker<Fp2Ops>, 1>(js, st);
      else known = false;
    }
    if (!known) return BH_ERR_INVALID_ARG;
    if (!ok) return BH_ERR_HIP;
  }
  return BH_OK;
}

// ============================================================================================
// host orchestration
// ============================================================================================
// F = the ops bundle the accumulation computes with (FpOps for G1; Fp2K3Ops, or single-lane Fp2Ops, for G2), FR the
// bundle of the merge and reduction kernels; records in memory are Affine / XYZZ over F::Mem == FR::Mem, so the two
// can differ: a big G2 job accumulates one lane per point (throughput) and reduces a window table's 2^15 buckets in
// lane triples (latency).
// Everything the stages after the sort read.  msm_enqueue fills it in, and a job issued with BH_MSM_HOLD keeps a copy of it
// (MsmJobImpl::resume) until it is started: plain values and raw device pointers.  The pointers all lie in the job's
// workspace block (job.dev_allocs, returned to the pool when the job is waited for) - except `gather`, which points into the
// base handle's memory: the registered vector, its 128-byte-stride copy or its window table.  The caller keeps the handle
// until the wait, and bh_ctx_trim leaves automatic tables alone while a job is in flight (api_context.hip).
template <class M>
struct AfterSort {
  MsmPlan p;
  MergePlan mp;
  ReducePlan rp;
  BaseView gather;             // MsmSources::gather: what the accumulate launch reads, and how far apart
  bool small_fused, lds_acc;   // the buckets are filled already (msm_small_fill_kernel); the accumulator lives in LDS
  const u64 *sorted;           // the sorted pairs (null when small_fused)
  const u32 *zstart;
  XYZZ<M> *pts, *head, *tail, *piece_out, *rowcol, *part, *bits;
  LongRun *long_runs;
  BigRun *big_runs;
  ErrFlags *err;               // ... and the start of what the job copies to its pinned result buffer: [status slot][bits]
  size_t result_bytes;
};
template <class F, class FR>
static int msm_after_sort(MsmJobImpl &job, const AfterSort<typename F::Mem> &s) {
  typedef typename F::Mem M;
  Context &c = *job.ctx;
  hipStream_t st = job.stream;
  const MsmPlan &p = s.p;
  // 4. accumulate equal chunks, then fold the buckets that straddle chunk boundaries
  if (s.small_fused) {
    if (job.timed) BH_HIP_CHECK(hipEventRecord(job.ev_accum, st));
  } else {
    const dim3 grid = accumulate_grid<F>(p);
    // launches that fill the chip join the context's accumulation chain (common.hpp)
    const bool chained = (u64)grid.x * grid.y * 128 >= (u64)c.num_cus * 4 * 64;
    std::unique_lock<std::mutex> chain_lock(c.acc_mu, std::defer_lock);
    if (chained) {
      if (!job.res.acc_event) BH_HIP_CHECK(hipEventCreateWithFlags(&job.res.acc_event, hipEventDisableTiming));
      chain_lock.lock();
      if (c.last_acc_event) BH_HIP_CHECK(hipStreamWaitEvent(st, c.last_acc_event, 0));
      for (hipEvent_t ev : c.pending_barriers) BH_HIP_CHECK(hipStreamWaitEvent(st, ev, 0));   // bh_ctx_accumulations_after
      c.pending_barriers.clear();
    }
    const Affine<M> *acc_bases = (const Affine<M> *)s.gather.ptr;
    if (int rc = launch_accumulate<F>(st, p, s.lds_acc, s.sorted, s.zstart, acc_bases, s.gather.stride, s.pts, s.head, s.tail, s.err)) return rc;
    if (chained) {
      BH_HIP_CHECK(hipEventRecord(job.res.acc_event, st));
      c.last_acc_event = job.res.acc_event;
      chain_lock.unlock();
    }
    if (job.timed) BH_HIP_CHECK(hipEventRecord(job.ev_accum, st));   // brackets exactly the accumulate launch
    const int rc = launch_merges<FR>(st, p, s.mp, c.num_cus, 0, s.sorted, s.zstart, s.pts, s.head, s.tail, s.long_runs, s.big_runs, s.piece_out, s.err);
    if (rc) return rc;
  }
  // 5. reduce: row and column sums, then the bit sums and totals the host tail combines (launch_reduce, above)
  if (int rc = launch_reduce<FR>(st, s.rp, s.pts, s.rowcol, s.part, s.bits)) return rc;
  if (job.timed) BH_HIP_CHECK(hipEventRecord(job.ev_end, st));
  // status words + results to pinned host memory, one copy: [ErrFlags slot (256 B)][bit sums]
  job.host_result_bytes = s.result_bytes;
  if (job.host_result_bytes > job.res.pinned_bytes) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipMemcpyAsync(job.host_result, s.err, job.host_result_bytes, hipMemcpyDeviceToHost, st));
  return BH_OK;
}
template <class F, class FR>
static int msm_enqueue(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                       const u64 *density_dev, const MsmOpts &opts) {
  typedef typename F::Mem M;
  static_assert(sizeof(typename FR::Mem::T) == sizeof(typename M::T), "both bundles work on the same records");
  typedef XYZZ<M> Pt;
  constexpr bool G2 = (M::WORDS == 24);
  Context &c = *job.ctx;
  hipStream_t st = job.stream;
  // running bucket sum in LDS: only meaningful for the single-lane G2 kernel (its default), or when forced
  const bool lds_acc = F::LANES == 1 && ((opts.flags & BH_MSM_ACC_LDS) ? true : (opts.flags & BH_MSM_ACC_REGISTERS) ? false : G2);
  // which plan, and which of the handle's sources each kernel reads (msm_types.hpp)
  const MsmSources src = msm_pick_sources(bases, opts, n, G2 ? BH_G2 : BH_G1,
                                          F::LANES != 1 ? ACC_MULTI_LANE : lds_acc ? ACC_ONE_LANE_LDS : ACC_ONE_LANE_REGISTERS);
  if (!src.valid) return BH_ERR_INVALID_ARG;
  const bool use_table = src.use_table;
  const u64 n_bases = bases.n;
  // a many-job: opts.vectors scalar vectors of n scalars, vector v at scalars_dev + v * opts.scalar_stride
  const bool many = opts.vectors > 1;
  if (many && (opts.flags & BH_MSM_HOLD)) return BH_ERR_INVALID_ARG;
  const MsmPlan p = many        ? make_many_plan(n, opts.vectors, use_table ? &bases.tab : nullptr, opts.c, opts.chunk, G2, c.num_cus)
                    : use_table ? make_table_plan(n, bases.tab, opts.chunk, G2, c.num_cus)
                                : make_plan(n, opts.c, opts.chunk, G2);
  job.plan = p;
  if ((u64)p.Wd * n >= ((u64)1 << 32)) return BH_ERR_INVALID_ARG;  // pair positions are 32-bit
  if (n_bases >= ((u64)1 << 31)) return BH_ERR_INVALID_ARG;        // base index shares its word with the sign bit
  if (many && !many_plan_valid(p, n_bases)) return BH_ERR_INVALID_ARG;

  // ---- one workspace block per job, carved into its buffers (one pool round trip, one memset) ----------
  const u64 npairs = many ? (u64)p.W * p.n : (u64)p.Wd * n;
  const u64 ncounts = sort_counts_elems(p);
  const u64 nslots = (u64)p.W * p.chunks_per_window;
  constexpr BundleGeom geom = bundle_geom<FR>();
  const MergePlan mp = merge_plan(p, geom, c.num_cus);
  const ReducePlan rp = reduce_plan(p, geom, c.num_cus);
  if (rp.overflow) return BH_ERR_INVALID_ARG;
  const u64 nwords = (n + 63) / 64;
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~size_t(255); return at; };
  // zero-initialised region first: status words, the result slots (so that both leave in ONE copy), then the buckets
  // (all-zero XYZZ == identity)
  const size_t bits_bytes = (size_t)rp.bits_elems * sizeof(Pt);   // per window: (c-1) bit sums U[w][p], then W plain totals T[w]
  const size_t o_err = carve(sizeof(ErrFlags));                // 256-byte slot
  const size_t o_bits = carve(bits_bytes);
  const size_t o_pts = carve((u64)p.NB * sizeof(Pt));
  const size_t zero_bytes = off;
  const size_t o_pairs_a = carve(npairs * 8), o_pairs_b = carve(npairs * 8);
  const size_t o_counts = carve((ncounts + 1) * 4), o_scan = carve(scan_tmp_elems(ncounts + 1) * 4), o_zstart = carve((u64)p.W * 4);
  const size_t o_head = carve(nslots * sizeof(Pt)), o_tail = carve(nslots * sizeof(Pt));
  const size_t o_long = carve((u64)mp.max_long * sizeof(LongRun)), o_big = carve((u64)mp.max_big * sizeof(BigRun));
  const size_t o_pieces = carve((u64)mp.max_pieces * sizeof(Pt));
  const size_t o_rowcol = carve(rp.rowcol_elems * sizeof(Pt));
  const bool want_part = rp.want_part;   // (the piece sums of the two-stage row / column sums: reduce_plan)
  const size_t o_part = want_part ? carve(rp.part_elems * sizeof(Pt)) : 0;
  const size_t o_prefix = density_dev ? carve((nwords + 1) * 4) : 0;
  char *ws = (char *)c.pool.acquire(off);
  if (!ws) return BH_ERR_HIP;
  job.dev_allocs.push_back(ws);
  MsmBuffers b;
  b.err = (ErrFlags *)(ws + o_err);
  b.pairs_a = (u64 *)(ws + o_pairs_a); b.pairs_b = (u64 *)(ws + o_pairs_b);
  b.counts = (u32 *)(ws + o_counts); b.scan_tmp = (u32 *)(ws + o_scan); b.zstart = (u32 *)(ws + o_zstart);
  b.word_prefix = density_dev ? (u32 *)(ws + o_prefix) : nullptr;
  Pt *pts = (Pt *)(ws + o_pts), *head = (Pt *)(ws + o_head), *tail = (Pt *)(ws + o_tail);
  LongRun *long_runs = (LongRun *)(ws + o_long);
  BigRun *big_runs = (BigRun *)(ws + o_big);
  Pt *piece_out = (Pt *)(ws + o_pieces);
  Pt *rowcol = (Pt *)(ws + o_rowcol), *bits = (Pt *)(ws + o_bits);
  Pt *part = want_part ? (Pt *)(ws + o_part) : nullptr;
  ErrFlags *err = b.err;
  job.err_dev = err;
  job.scalars_dev = scalars_dev; job.density_dev = density_dev; job.word_prefix = b.word_prefix;
  job.resolve_bases = src.resolve;
  job.skip = skip; job.n_bases = n_bases; job.fmt = fmt;
  job.ref_n = opts.ref_n; job.always_resolve_ident = opts.always_resolve_ident;

  job.timed = (opts.flags & BH_MSM_STAGE_TIMES) != 0;
  if (job.timed) BH_HIP_CHECK(hipEventRecord(job.ev_begin, st));
  BH_HIP_CHECK(hipMemsetAsync(ws, 0, zero_bytes, st));
  const u64 *sorted = nullptr;
  // small multiexps over a window table: one launch for everything up to the filled buckets (small_fill_plan has the gate)
  const SmallFillPlan sp = small_fill_plan(p, src.small_path, many, opts.flags, small_fill_workers<F>());
  const bool small_fused = sp.fused;
  if (small_fused) {
    int rc = launch_small_fill<F>(st, p, sp, scalars_dev, fmt, density_dev, b.word_prefix, (u64)skip, (u64)n_bases,
                                  (const Affine<M> *)src.gather.ptr, pts, err);
    if (rc) return rc;
  } else {
    int rc = msm_run_stages(p, b, scalars_dev, fmt, density_dev, skip, n_bases, st, &sorted, opts.scalar_stride);
    if (rc) return rc;
  }
  if (job.timed) BH_HIP_CHECK(hipEventRecord(job.ev_sorted, st));
  // the pinned result buffer of a job's resources holds every single-vector plan; a many-job's W * c bit sums may not
  // fit: the job's resources grow to what its plan needs (and keep it when they are recycled)
  if (job_result_bytes(p, sizeof(Pt)) != (o_bits - o_err) + bits_bytes) return BH_ERR_INVALID_ARG;   // (bh_msm_many_plan_info reports it)
  if (many && job_result_bytes(p, sizeof(Pt)) > job.res.pinned_bytes) {
    const size_t want = (job_result_bytes(p, sizeof(Pt)) + 65535) & ~size_t(65535);
    void *bigger = nullptr;
    BH_HIP_CHECK(hipHostMalloc(&bigger, want, hipHostMallocDefault));
    (void)hipHostFree(job.res.pinned);
    job.res.pinned = bigger;
    job.res.pinned_bytes = want;
    job.host_result = bigger;
  }
  const bool hold = (opts.flags & BH_MSM_HOLD) != 0;
  if (hold) {
    // the digit / sort stage of a held job joins the barrier set of the accumulation chain: whichever accumulation is
    // started first waits for the sorts of ALL jobs issued so far (create_proof issues its multiexps held, then starts
    // them in chain order - no sort runs beside an accumulation and steals its SIMDs)
    if (!job.res.sort_event) BH_HIP_CHECK(hipEventCreateWithFlags(&job.res.sort_event, hipEventDisableTiming));
    BH_HIP_CHECK(hipEventRecord(job.res.sort_event, st));
    std::lock_guard<std::mutex> g(c.acc_mu);
    if (c.pending_barriers.size() < 32) c.pending_barriers.push_back(job.res.sort_event);
  }
  // everything after the sort: run now, or when the job is started (bh_msm_start / its wait)
  const AfterSort<M> after = {p, mp, rp, src.gather, small_fused, lds_acc, sorted, b.zstart, pts, head, tail, piece_out, rowcol, part,
                             bits, long_runs, big_runs, err, (o_bits - o_err) + bits_bytes};
  if (!hold) return msm_after_sort<F, FR>(job, after);
  job.resume = [after](MsmJobImpl &j) { return msm_after_sort<F, FR>(j, after); };
  return BH_OK;
}

// host tail: result = sum_w 2^(c*w) (sum_p 2^p U[w][p] + T[w])
//   bits layout: [W][lo_bits] column-bit sums, [W][hi_bits] row-bit sums, [W] window totals
template <class F>
static void msm_host_tail(const MsmPlan &p, const XYZZ<F> *bits_dev_layout, void *out_dev_layout) {
  typedef typename HostOf<F>::type H;   // 64-bit-limb host arithmetic, identical record layout
  static_assert(sizeof(XYZZ<H>) == sizeof(XYZZ<F>) && sizeof(Affine<H>) == sizeof(Affine<F>), "layout");
  // the device kernels hand over lazily reduced coordinates ([0, 2p), ff.cuh); the host arithmetic wants
  // canonical ones
  std::vector<XYZZ<F>> canon(bits_dev_layout, bits_dev_layout + (size_t)p.W * p.c);
  for (XYZZ<F> &q : canon) { F::canon(q.x); F::canon(q.y); F::canon(q.zz); F::canon(q.zzz); }
  const XYZZ<H> *bits = reinterpret_cast<const XYZZ<H> *>(canon.data());
  XYZZ<H> acc;
  xyzz_set_identity(acc);
  const u32 cb = p.c - 1;
  const XYZZ<H> *lo = bits, *hi = bits + (size_t)p.W * p.lo_bits, *tot = bits + (size_t)p.W * cb;
  for (int w = (int)p.W - 1; w >= 0; w--) {
    for (int b = (int)p.c - 1; b >= 0; b--) {
      XYZZ<H> t;
      xyzz_dbl(t, acc);
      acc = t;
      if (b < (int)cb) {
        const XYZZ<H> &u = (b >= (int)p.lo_bits) ? hi[(size_t)w * p.hi_bits + (b - p.lo_bits)]
                                                 : lo[(size_t)w * p.lo_bits + b];
        xyzz_add(t, acc, u);
        acc = t;
      }
      if (b == 0) {   // the "+1" of the bucket weights
        xyzz_add(t, acc, tot[w]);
        acc = t;
      }
    }
  }
  Affine<H> res;   // caller buffers carry no alignment guarantee: go through an aligned local
  xyzz_to_affine(res, acc);
  memcpy(out_dev_layout, &res, sizeof res);
}

// many-plan: the tail over vector v's windows only.  launch_reduce lays the bit sums out window-major over ALL W sets
// ([W][lo_bits], [W][hi_bits], [W]); the vector's slice of each part, put side by side, is exactly what the tail above
// reads for a plan of windows_per_vector sets (table flavour: one set, c doublings).
template <class F>
static void msm_host_tail_vector(const MsmPlan &p, u32 v, const XYZZ<F> *bits_dev_layout, void *out_dev_layout) {
  MsmPlan pv = p;
  pv.vectors = 1;
  pv.W = p.windows_per_vector;
  pv.NB = pv.W * p.nb;
  const u32 cb = p.c - 1;
  const size_t w0 = (size_t)v * pv.W;
  std::vector<XYZZ<F>> slice((size_t)pv.W * p.c);
  const XYZZ<F> *lo = bits_dev_layout, *hi = bits_dev_layout + (size_t)p.W * p.lo_bits, *tot = bits_dev_layout + (size_t)p.W * cb;
  std::copy(lo + w0 * p.lo_bits, lo + (w0 + pv.W) * p.lo_bits, slice.begin());
  std::copy(hi + w0 * p.hi_bits, hi + (w0 + pv.W) * p.hi_bits, slice.begin() + (size_t)pv.W * p.lo_bits);
  std::copy(tot + w0, tot + w0 + pv.W, slice.begin() + (size_t)pv.W * cb);
  msm_host_tail<F>(pv, slice.data(), out_dev_layout);
}

template <class F>
static int msm_finish(MsmJobImpl &job, void *out_affine, float *ms) {
  Context &c = *job.ctx;
  int rc = BH_OK;
  if (job.trivial) {
    memset(out_affine, 0, sizeof(Affine<F>));
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    return job.early_rc;
  }
  if (job.resume) {   // held and never started: start it now
    rc = job.resume(job);
    job.resume = nullptr;
  }
  if (hipStreamSynchronize(job.stream) != hipSuccess) rc = BH_ERR_HIP;
  if (rc == BH_OK) {
    const MsmPlan &p = job.plan;
    constexpr size_t ERR_SLOT = 256;   // the carve granularity of msm_enqueue
    ErrFlags ef;
    memcpy(&ef, job.host_result, sizeof ef);
    if (ms) {  // [0] whole device pipeline, [1] digits+sort, [2] bucket accumulation, [3] reductions
      ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
      if (job.timed) {
        (void)hipEventElapsedTime(&ms[0], job.ev_begin, job.ev_end);
        (void)hipEventElapsedTime(&ms[1], job.ev_begin, job.ev_sorted);
        (void)hipEventElapsedTime(&ms[2], job.ev_sorted, job.ev_accum);
        (void)hipEventElapsedTime(&ms[3], job.ev_accum, job.ev_end);
      }
    }
    job.saw_eof = ef.eof != 0;
    job.saw_ident = ef.ident != 0;
    // [0] sorted entries  [1] zero digits among them  [2] mixed additions of the accumulate launch  [3] chunk lanes
    // [4] window bits c  [5] chunk length K  [6] windows W (1: window-table plan)  [7] digit columns per scalar
    job.done_stats[0] = (u64)p.W * p.n; job.done_stats[1] = ef.zeros; job.done_stats[2] = ef.madds;
    job.done_stats[3] = (u64)p.W * p.chunks_per_window; job.done_stats[4] = p.c; job.done_stats[5] = p.chunk;
    job.done_stats[6] = p.W; job.done_stats[7] = p.Wd;
    if (p.vectors > 1) {
      // many-job: the flags are per job - with either set every vector is answered by the single-vector path
      // (bh_msm_many_wait), which gives each its own code with the reference's precedence
      job.many_out.assign((size_t)p.vectors * sizeof(Affine<F>), 0);
      job.many_fallback = ef.eof || ef.ident;
      if (!job.many_fallback)
        for (u32 v = 0; v < p.vectors; v++)
          msm_host_tail_vector<F>(p, v, (const XYZZ<F> *)((const char *)job.host_result + ERR_SLOT),
                                  job.many_out.data() + (size_t)v * sizeof(Affine<F>));
      memset(out_affine, 0, sizeof(Affine<F>));
    } else if (ef.ident && (ef.eof || job.always_resolve_ident)) {
      // both kinds of failure exist (or the caller folds shards): the reference reports the top window's first failure
      const u64 nref = job.ref_n ? job.ref_n : p.nd;
      const u32 lo_ref = err_resolve_lo_ref(nref);   // (msm_stage_plans.hpp)
      if (launch_err_resolve<F>(job.stream, job.scalars_dev, job.fmt, p.nd, job.density_dev, job.word_prefix, job.skip, job.n_bases,
                                (const Affine<F> *)job.resolve_bases.ptr, job.resolve_bases.stride, lo_ref, job.err_dev) != BH_OK ||
          hipMemcpyAsync(&ef, job.err_dev, sizeof ef, hipMemcpyDeviceToHost, job.stream) != hipSuccess ||
          hipStreamSynchronize(job.stream) != hipSuccess)
        rc = BH_ERR_HIP;
      else {
        job.saw_ident_top = ef.ident_top != 0;
        rc = !ef.eof ? BH_ERR_UNEXPECTED_IDENTITY : ef.ident_top ? BH_ERR_UNEXPECTED_IDENTITY : BH_ERR_UNEXPECTED_EOF;
      }
    } else if (ef.eof) {
      rc = BH_ERR_UNEXPECTED_EOF;
    } else if (ef.ident) {
      rc = BH_ERR_UNEXPECTED_IDENTITY;
    } else {
      msm_host_tail<F>(p, (const XYZZ<F> *)((const char *)job.host_result + ERR_SLOT), out_affine);
    }
  }
  for (void *ptr : job.dev_allocs) c.pool.release(ptr);
  job.dev_allocs.clear();
  return rc;
}

// OPS = the record format in memory (FpOps / Fp2Ops).  msm_enqueue_<group> itself (which kernel bundle accumulates,
// which one merges and reduces) is written out in msm_g1.hip / msm_g2.hip.
#define BH_INSTANTIATE_MSM_SUPPORT(SUFFIX, OPS)                                                               \
  int window_table_##SUFFIX(BaseView src, void *dst, u32 dst_stride, u64 n, u32 c, u32 W, hipStream_t st) {   \
    return window_table_t<OPS>(src, dst, dst_stride, n, c, W, st);                                            \
  }                                                                                                           \
  int msm_finish_##SUFFIX(MsmJobImpl &job, void *out_affine, float *ms) {                                     \
    return msm_finish<OPS>(job, out_affine, ms);                                                              \
  }                                                                                                           \
  int fixed_base_mul_##SUFFIX(const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev,  \
                              hipStream_t st, void *table_dev) {                                              \
    return fixed_base_mul_t<OPS>(base_host, scalars_dev, n, fmt, out_dev, st, table_dev);                     \
  }                                                                                                           \
  int points_check_##SUFFIX(const void *pts_dev, u64 n, u32 *status_dev, hipStream_t st) {                    \
    return points_check_t<OPS>(pts_dev, n, status_dev, st);                                                   \
  }                                                                                                           \
  void host_point_add_##SUFFIX(void *r, const void *a, const void *b, u64 n) {                                \
    host_point_add_t<OPS>(r, a, b, n);                                                                        \
  }                                                                                                           \
  void host_point_mul_##SUFFIX(void *r, const void *a, const void *k) {                                       \
    host_point_mul_t<OPS>(r, a, (const u32 *)k);                                                              \
  }                                                                                                           \
  void host_point_lincomb_##SUFFIX(void *r, const void *pts, const void *scalars, u64 n) {                    \
    host_point_lincomb_t<OPS>(r, pts, (const u32 *)scalars, n);                                               \
  }

}  // namespace bh
