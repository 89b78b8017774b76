// Host plans of stages 4 and 5 of a multiexp: whether a job takes the one-launch small path and that launch
// (small_fill_plan), the merge parameters and queue bounds (merge_plan), the reduction's buffer sizes and its whole launch
// schedule (reduce_plan), and the top window of the error-resolution pass (err_resolve_lo_ref) - pure functions of a plan, a
// bundle's geometry and the chip's CU count.
// Plain C++: no HIP call, no device function, no field or point type.  The kernels these plans are for live in
// msm_accumulate.cuh, msm_merge.cuh and msm_sums.cuh; msm_merge.cuh derives a bundle's BundleGeom from its worker types
// (bundle_geom<FR>()), and msm_ec.cuh launches what the plans say.  Tests read the plans through bh_test_small_fill_plan /
// bh_test_merge_plan / bh_test_reduce_plan / bh_test_err_resolve_lo_ref.
#pragma once
#include <algorithm>
#include <cmath>

#include "msm_types.hpp"

namespace bh {

// Worker kinds of the sum and merge kernels (the forms of bh_test_sum_jobs_dev): a full point per lane / lane pair / lane
// triple (XyzzWorker<F>), or half a point per lane (G1, K2Worker) / per lane triple (G2, K6Worker)
enum : u32 { WK_XYZZ_FP = 0, WK_K2 = 1, WK_XYZZ_FP2 = 2, WK_XYZZ_FP2K3 = 3, WK_XYZZ_FP2PAIR = 4, WK_K6 = 5, WK_NONE = 0xffffffffu };
// What the planners read from the bundle FR of the merge and reduction kernels
struct BundleGeom {
  u32 full_kind;                 // XyzzWorker<FR>
  u32 per_wave, solo_per_wave;   // ... its workers per wavefront in shuffle trees / where every worker sums alone
  u32 lanes;                     // ... lanes per worker (FR::LANES)
  u32 sum_waves;                 // wavefronts per workgroup of its sum kernel
  u32 half_kind, half_per_wave;  // the group's half-point worker: WK_K2 / WK_K6, or WK_NONE and 0 (one-lane G2)
  u32 long_piece;                // partials per piece of a big run, on the worker that folds the pieces
  bool g2;
};

// ============================================================================================
// stages 1 - 4 in one launch: which multiexps take msm_small_fill_kernel (msm_accumulate.cuh), and its launch
// ============================================================================================
constexpr u32 SMALL_MAX_SCALARS = 2048, SMALL_MAX_ENTRIES = 20480 + 1024, SMALL_MAX_PER_BUCKET = 16, SMALL_LIST_CAP = 24;
constexpr u32 SMALL_THREADS = 256, SMALL_LANES_PER_BUCKET = 4;
// dynamic LDS of the kernel: base indices, digit table, per-bucket entry lists of the workgroup's buckets
inline size_t small_fill_lds_bytes(u32 nd, u32 n_entries) {
  return (size_t)nd * 4 + (((size_t)n_entries * 2 + 3) & ~size_t(3)) + SMALL_THREADS * 4 + (size_t)SMALL_THREADS * SMALL_LIST_CAP * 2;
}
struct SmallFillPlan {
  bool fused;                  // the job takes the one-launch path; the rest describes that launch
  u32 workgroups, threads;
  size_t lds_bytes;
  u32 buckets_per_workgroup;   // workers_per_workgroup / SMALL_LANES_PER_BUCKET
  u32 top_bits;                // bits of a scalar that reach the table's top row
  u64 sliver_load;             // entries the top row alone is expected to send to each of its 2^top_bits buckets
};
// small multiexps over a window table: one launch for everything up to the filled buckets (msm_small_fill_kernel)
// ... and only when no bucket is EXPECTED to outgrow its list: rows whose top one is a sliver of t = 255 - (Wd - 1) c bits (10-bit
// rows: t = 5, 11 bits: 2, 12 bits: 3) send the top digit of every scalar to 2^t buckets, nd / 2^t entries each - such buckets fall
// back to a scan of the whole digit table per worker (an explicit 11-bit table over 2^9 points took 8.9 ms in this kernel against
// 0.7 through the sort: profiles/r6_call54_tiny_g2_bits.txt); the default 13-bit tables have t = 8
// What each term keeps the kernel inside: nd <= SMALL_MAX_SCALARS - its density prefix walks at most 32 words per scalar;
// n <= SMALL_MAX_ENTRIES and the LDS bound - base indices, digits and lists fit a workgroup's 64 KiB, and an entry id its list's
// 16 bits; c <= 15 - a digit, up to 2^(c-1) in magnitude, fits a `short`; one bucket set of one vector - the kernel has no other.
// small_path: MsmSources::small_path; many: the job holds several scalar vectors; flags: MsmOpts::flags;
// workers_per_workgroup: workers_per_block<F>(SMALL_THREADS, tree_per_wave<F>()) of the bundle F that accumulates
inline SmallFillPlan small_fill_plan(const MsmPlan &p, bool small_path, bool many, u32 flags, u32 workers_per_workgroup) {
  SmallFillPlan s;
  s.top_bits = 255u - (p.Wd - 1) * p.c;
  s.sliver_load = s.top_bits >= 31 ? 0 : ((u64)p.nd >> s.top_bits);
  s.lds_bytes = small_fill_lds_bytes(p.nd, p.n);
  s.fused = small_path && plan_fused_sort(p) && !many && p.nd <= SMALL_MAX_SCALARS && p.n <= SMALL_MAX_ENTRIES &&
            (u64)p.n <= (u64)SMALL_MAX_PER_BUCKET * p.nb && p.c <= 15 && s.lds_bytes <= 64 * 1024 &&
            s.sliver_load + (u64)p.n / p.nb <= SMALL_LIST_CAP / 2 && !(flags & BH_MSM_NO_SMALL_PATH);
  s.threads = SMALL_THREADS;
  s.buckets_per_workgroup = workers_per_workgroup / SMALL_LANES_PER_BUCKET;
  s.workgroups = s.buckets_per_workgroup ? (p.nb + s.buckets_per_workgroup - 1) / s.buckets_per_workgroup : 0;
  return s;
}

// ============================================================================================
// the error-resolution pass (msm_err_resolve_kernel): where the reference's top window starts
// ============================================================================================
// The reference sizes its windows by the number of exponents, c = 3 below 32 of them and ceil(ln n) from there on
// (multiexp.rs:318-322), and reports the first failure of its top window: bits [lo_ref, 256) of a scalar
inline u32 err_resolve_lo_ref(u64 nref) {
  const double c_ln = (nref < 32) ? 3.0 : std::ceil(std::log((double)nref));
  const u32 c_ref = (u32)c_ln, w_ref = (255 + c_ref - 1) / c_ref;
  return c_ref * (w_ref - 1);
}

// ============================================================================================
// stage 4: the merge parameters of a plan and the queue bounds
// ============================================================================================
struct MergeBounds {
  u32 max_long, max_big, max_pieces;   // entries of long_runs, big_runs, piece_out
};
struct MergePlan {
  u32 walk;            // the owner lane of a run folds at most this many following chunks itself
  u32 run_lanes;       // G workers per queued medium run
  bool runs_on_pairs;  // ... on the group's half-point worker
  u32 big_chunks;      // runs of more following chunks than this are cut into pieces
  u32 piece;           // partials per piece
  u32 max_long, max_big, max_pieces;
};
// Upper bounds of what msm_merge_chunks_kernel can queue over nslots chunks (all windows).  A queued run owns the chunks
// [lane, last) alone - its last chunk may be the first of the next run - so a run of more than `walk` following chunks
// takes at least walk + 1 chunks out of nslots, a big one big_chunks + 1.
// Pieces: sum of ceil(L_r / piece) over the big runs: consecutive runs share one chunk, so sum L_r <= nslots + max_big
inline MergeBounds merge_bounds(u64 nslots, u32 walk, u32 big_chunks, u32 piece) {
  MergeBounds b;
  b.max_long = (u32)(nslots / (walk + 1) + 1);
  b.max_big = (u32)(nslots / (big_chunks + 1) + 1);
  b.max_pieces = (u32)((nslots + b.max_big) / piece + b.max_big + 1);
  return b;
}
inline MergePlan merge_plan(const MsmPlan &p, const BundleGeom &geom, int num_cus) {
  const bool G2_SEXTETS = geom.half_kind == WK_K6, PAIRS_POSSIBLE = geom.half_kind != WK_NONE;   // "pairs" below: the half-point worker of the group
  MergePlan mp;
  // the owner lane of a run folds at most `walk` following chunks itself; longer runs are queued for
  // msm_merge_runs_kernel (G workers per run), the longest of those for the workgroup kernel
  mp.walk = 4;
  // G workers per queued run: 8-16 chunk runs become 1-2 serial additions + 3 tree levels; when the AVERAGE run is
  // much longer than that (window tables over tiny vectors: 32 n entries in 128 buckets, chunks of 8) more workers
  // shorten the chain as long as the launch still fits the chip
  // [r6] G1: the same on lane PAIRS (K2: half the latency of an addition for twice the lanes) when that is cheaper by
  // the same model - levels x latency of a level x how far the launch overfills the chip
  // [r6] G2 in lane triples: the same on lane SEXTETS (K6Worker)
  const double LEVEL_US = G2_SEXTETS ? 37.0 : 19.0, HALF_LEVEL_US = G2_SEXTETS ? 20.0 : 10.5;   // a tree level, by worker kind
  u32 run_lanes = 8;
  bool runs_on_pairs = false;
  {
    const double avg_chunks = (double)p.n / (double)p.nb / (double)p.chunk;   // per window: n sorted entries, nb buckets
    double best_cost = 1e30;
    auto sweep = [&](u32 per_wave, double level_us, bool pairs) {
      for (u32 g = 8, lg = 3; g <= per_wave; g <<= 1, lg++) {
        const double steps = std::ceil(std::max(1.0, avg_chunks) / g) + lg;
        const double waves = (double)p.NB * g / (double)per_wave;
        const double cost = steps * level_us * std::max(1.0, waves / ((double)num_cus * 4));
        if (cost < best_cost) { best_cost = cost; run_lanes = g; runs_on_pairs = pairs; }
      }
    };
    sweep(geom.per_wave, LEVEL_US, false);
    if (PAIRS_POSSIBLE) sweep(geom.half_per_wave, HALF_LEVEL_US, true);
    // (the model takes every bucket for a queued run - true of window-table plans; where a typical bucket fits a chunk only
    // the few outliers are queued and the chip has the lanes)
    if (PAIRS_POSSIBLE && avg_chunks <= 1.0) { run_lanes = 8; runs_on_pairs = true; }
  }
  mp.run_lanes = run_lanes;
  mp.runs_on_pairs = runs_on_pairs;
  // runs of more than big_chunks chunks - more than four serial additions per worker of msm_merge_runs_kernel - are cut
  // into workgroup-sized pieces (msm_merge_long_kernel) that run on the group's half-point worker (G1: lane pairs)
  // ... but never a run that is merely TYPICAL: where the average bucket already spans dozens of chunks (32 rows of 8 bits over
  // 2^11 G2 points: 64 chunks per bucket) "big" starts at twice the average (round 6, first cut: half of that table's runs
  // went down the long path, 0.81 -> 1.06 ms)
  mp.big_chunks = std::max(std::max(32u, 4u * run_lanes), (u32)(2.0 * (double)p.n / (double)p.nb / (double)p.chunk));
  mp.piece = geom.long_piece;
  const MergeBounds mb = merge_bounds((u64)p.W * p.chunks_per_window, mp.walk, mp.big_chunks, mp.piece);
  mp.max_long = mb.max_long; mp.max_big = mb.max_big; mp.max_pieces = mb.max_pieces;
  return mp;
}

// ============================================================================================
// stage 5: what msm_enqueue carves for the reduction, and every launch of it
// ============================================================================================
// workers of a wavefront in a job of `lanes` workers per output: per_wave (a power of two for the trees) - but all of
// solo_per_wave when every worker sums alone, the first stage of a two-stage sum on lane triples [r6]: 84 per workgroup
constexpr u32 sum_workers_per_wave(u32 per_wave, u32 solo_per_wave, u32 lanes) {
  return (solo_per_wave != per_wave && lanes == 1) ? solo_per_wave : per_wave;
}
// The one place that counts: clamps a job's workers per output to what a workgroup of `nwaves` wavefronts holds; returns
// the job's workgroups
inline u32 sum_job_blocks(SumDesc &d, u32 per_wave, u32 solo_per_wave, u32 nwaves) {
  if (d.lanes > nwaves * per_wave) d.lanes = nwaves * per_wave;
  const u32 wpb = nwaves * sum_workers_per_wave(per_wave, solo_per_wave, d.lanes);
  return (u32)(((u64)d.groups * d.lanes + wpb - 1) / wpb);
}

// the buffers of the reduction: the filled buckets; [W][H] row sums, then [W][Lw] column sums; the piece sums of the
// two-stage row / column sums; the result slots
enum : u32 { RB_PTS, RB_ROWCOL, RB_PART, RB_BITS, RB_BUFS };
struct ReduceJob {
  SumDesc d;             // (groups == 0: nothing to do)
  u32 nblocks;           // workgroups assigned to this job
  u32 in_buf, out_buf;   // RB_*: it reads records of in_buf from in_off on and writes those of out_buf from out_off on
  u64 in_off, out_off;
};
// up to three independent reductions per launch (rows + columns, then the bit-sum sets and the plain window totals): they
// are latency-bound, so sharing a launch lets the hardware overlap them
struct ReduceLaunch {
  u32 kind, waves;   // worker kind (WK_*), wavefronts per workgroup
  u32 blocks;        // workgroups of the launch: the sum over its jobs
  ReduceJob j[3];
};
// rows and columns - in one launch, or in two stages of one launch each - then the bit sums and totals (reduce_plan)
constexpr u32 REDUCE_ROWCOL_LAUNCHES = 2, REDUCE_BITS_LAUNCHES = 1, REDUCE_MAX_LAUNCHES = REDUCE_ROWCOL_LAUNCHES + REDUCE_BITS_LAUNCHES;
static_assert(REDUCE_MAX_LAUNCHES <= 8, "tests query a reduction's launches into room for eight");
struct ReducePlan {
  u32 two_len;      // elements per piece of the two-stage row / column sums
  bool want_part;   // ... which this plan takes
  u64 rowcol_elems, part_elems, bits_elems;   // records of `rowcol` ([W][H] row sums, [W][Lw] column sums), `part`, `bits`
  u32 n_launches;
  ReduceLaunch launch[REDUCE_MAX_LAUNCHES];   // in order; a launch with nothing to do is left out
  bool overflow;    // a launch found no room (a planner outgrew REDUCE_MAX_LAUNCHES): the plan is refused, not run short
};

// workers per output: minimise (serial adds per worker + tree depth) x (waves per SIMD, at least 1);
// these kernels are latency-bound chains of point additions, not throughput-bound.
inline u32 pick_lanes(const BundleGeom &geom, int num_cus, u32 groups, u32 count) {
  const u32 NW = geom.sum_waves, PW = NW * geom.per_wave;   // workers per workgroup of the full worker's kernel: 64
  // wavefront slots the launch may fill before a step stretches: ONE resident wavefront per SIMD - a second does not
  // interleave for free in these mad-bound chains (G1 2^17-2^20 reduce 0.73-0.99 ms modelled with 1, 0.92-1.19 ms with 2; G2
  // within noise: profiles/archive/r2_call8_slots.txt); a block of lane triples is four wavefronts
  const double slots = (double)num_cus * 4;
  u32 best = 1;
  double best_cost = 1e30;
  for (u32 g = 1, lg = 0; g <= PW; g <<= 1, lg++) {
    if (g > count && g > 1) break;
    // a lane-triple group wider than one wavefront pays two barriers and an LDS round trip (measured: ~2 additions)
    const double steps = (double)((count + g - 1) / g) + lg + ((geom.lanes == 3 && g > 16) ? 2.0 : 0.0);
    const double waves = (double)groups * g / (double)PW * (double)NW;
    const double cost = steps * std::max(1.0, waves / slots);
    if (cost < best_cost) { best_cost = cost; best = g; }
  }
  return best;
}
// a job with the lane count that suits its own groups and count
inline ReduceJob reduce_job(const BundleGeom &geom, int num_cus, u32 in_buf, u64 in_off, u32 out_buf, u64 out_off, SumDesc d) {
  d.lanes = d.groups ? pick_lanes(geom, num_cus, d.groups, d.mode == SUM_BITS ? std::max(1u, d.count / 2) : d.count) : 1;
  return ReduceJob{d, 0u, in_buf, out_buf, in_off, out_off};
}
// a launch of two jobs (the third: a copy of the second with nothing to do)
inline ReduceLaunch reduce_pair(const ReduceJob &a, const ReduceJob &b) {
  ReduceLaunch l{};
  l.j[0] = a; l.j[1] = b; l.j[2] = b; l.j[2].d.groups = 0;
  return l;
}
// clamps the launch's jobs to `nwaves` wavefronts of a worker kind and counts their workgroups; returns the total
inline u32 reduce_count(ReduceLaunch &l, u32 per_wave, u32 solo_per_wave, u32 nwaves) {
  l.blocks = 0;
  for (int q = 0; q < 3; q++) l.blocks += l.j[q].nblocks = sum_job_blocks(l.j[q].d, per_wave, solo_per_wave, nwaves);
  return l.blocks;
}
// Which worker kind a launch runs on, and its workgroups.  G1 launches that leave at least half of the SIMDs empty run on
// lane pairs (K2): half the latency per addition for twice the lanes.
// (the first stage of a two-stage sum chooses for itself: lane pairs in G1, the full worker in G2)
enum SumForce { SUMS_BY_RULE = 0, SUMS_ON_PAIRS = 1, SUMS_ON_FULL = 2 };
inline void reduce_choose_worker(const BundleGeom &geom, int num_cus, ReduceLaunch &l, SumForce force) {
  if (geom.half_kind == WK_K2) {
    constexpr double K2_SUM_FILL = 4.0;   // wavefronts per SIMD the lane-pair launch may reach
    // [r6] a handful of long sums (the bit sums and the total of ONE big bucket set): one workgroup of several
    // wavefronts per output
    u32 groups_all = 0, max_sel = 0;
    for (int q = 0; q < 3; q++)
      if (l.j[q].d.groups) {
        groups_all += l.j[q].d.groups;
        max_sel = std::max(max_sel, l.j[q].d.mode == SUM_BITS ? l.j[q].d.count / 2 : l.j[q].d.count / l.j[q].d.splits);
      }
    if (force == SUMS_BY_RULE && max_sel >= 128 && groups_all <= 2u * (u32)num_cus) {
      // (never more than four wavefronts: a CU has four SIMDs, and the wavefronts of a workgroup that share one take turns -
      // eight were 198 us for 2 + 5 + 3 levels, profiles/r6_call32_timeline.txt)
      const bool four = 2 * 64 < max_sel;
      l.kind = WK_K2; l.waves = four ? 4 : 2;
      for (int q = 0; q < 3; q++) l.j[q].d.lanes = l.waves * geom.half_per_wave;
      reduce_count(l, geom.half_per_wave, geom.half_per_wave, l.waves);
      return;
    }
    // (the one-lane launch would be single wavefronts)
    if (force != SUMS_ON_FULL &&
        (force == SUMS_ON_PAIRS || (double)reduce_count(l, geom.per_wave, geom.solo_per_wave, geom.sum_waves) * 2 <= K2_SUM_FILL * (double)num_cus * 4)) {
      l.kind = WK_K2; l.waves = 1;
      reduce_count(l, geom.half_per_wave, geom.half_per_wave, 1);
      return;
    }
  }
  if (geom.half_kind == WK_K6) {
    // G2: the same idea on lane sextets (32 workers per 256-thread block) while the launch stays within one wavefront per SIMD
    constexpr double K6_SUM_FILL = 8.0;   // blocks per CU the launch may reach
    ReduceLaunch k6 = l;
    if (force != SUMS_ON_FULL && (double)reduce_count(k6, geom.half_per_wave, geom.half_per_wave, 4) <= K6_SUM_FILL * (double)num_cus) {
      l = k6;
      l.kind = WK_K6; l.waves = 4;
      return;
    }
  }
  l.kind = geom.full_kind; l.waves = geom.sum_waves;
  reduce_count(l, geom.per_wave, geom.solo_per_wave, geom.sum_waves);
}
inline void reduce_add_launch(ReducePlan &rp, const BundleGeom &geom, int num_cus, ReduceLaunch l, SumForce force = SUMS_BY_RULE) {
  reduce_choose_worker(geom, num_cus, l, force);
  if (!l.blocks) return;
  if (rp.n_launches == REDUCE_MAX_LAUNCHES) { rp.overflow = true; return; }
  rp.launch[rp.n_launches++] = l;
}
// single-lane G2 (one resident wavefront per SIMD, so sharing a SIMD doubles every step): the row and the column job share
// one launch, choose their lane counts jointly - the launch lasts as long as its longest chain, stretched by
// how many wavefronts each SIMD has to interleave.  (With two wavefronts per SIMD - G1, K3-form G2 - they
// interleave almost for free and the per-job choice of pick_lanes is better.)
inline void pick_lanes_jointly(int num_cus, SumDesc &dr, SumDesc &dc) {
  const double simds = (double)num_cus * 4;
  double best = 1e30;
  u32 best_r = dr.lanes, best_c = dc.lanes;
  for (u32 gr = 1, lr = 0; gr <= 64 && gr <= std::max(1u, dr.count); gr <<= 1, lr++)
    for (u32 gc = 1, lc = 0; gc <= 64 && gc <= std::max(1u, dc.count); gc <<= 1, lc++) {
      const double steps = std::max((double)((dr.count + gr - 1) / gr) + lr, (double)((dc.count + gc - 1) / gc) + lc);
      const double waves = ((double)dr.groups * gr + (double)dc.groups * gc) / 64.0;
      const double cost = steps * std::max(1.0, waves / simds);
      if (cost < best) { best = cost; best_r = gr; best_c = gc; }
    }
  dr.lanes = best_r;
  dc.lanes = best_c;
}
// [r6] G1, bucket sets of 2^17 ... 2^21 points (16 windows of 2^15, or the 2^19 buckets of a 20-bit window table): one launch
// gives every output 16-32 lane pairs - 8-16 serial additions, then a 4-5 level tree in which half, a quarter, ...
// of the lanes work: 12-13 levels at four wavefronts per SIMD of which 61 % is useful work (0.50 ms for the 2^20 additions
// of a 2^20-term multiexp, 0.27 at the multiplier's throughput).  Two stages instead: (1) every output is cut into pieces
// of `len` consecutive elements and ONE worker adds up a piece - no tree, every lane busy - sized so that the launch is
// two wavefronts per SIMD; (2) the handful of piece sums per output are folded by a small tree launch.
// dr, dc: the row and the column sums in one stage; rows, cols: where their outputs start in rowcol
inline void reduce_two_stage(ReducePlan &rp, const BundleGeom &geom, int num_cus, const SumDesc &dr, const SumDesc &dc, u64 rows, u64 cols) {
  // G1: stage one on lane pairs.  G2 (lane triples): on the lane-triple kernel (16 workers per wavefront; sextets halve
  // that again and were within noise - reduce 1.89 / 1.96 ms against 1.86 / 1.97 at 2^19 / 2^20, profiles/r6_call42_g2_stage1.txt)
  const bool one_lane = geom.g2;
  const u32 Lw = dr.count, H = dc.count;
  const u32 len_r = std::min(rp.two_len, Lw), len_c = std::min(rp.two_len, H);
  const u32 Sr = Lw / len_r, Sc = H / len_c;
  const u64 part_r = 0, part_c = (u64)dr.groups * Sr;   // inside part
  SumDesc r1 = dr, c1 = dc;
  r1.splits = Sr; r1.groups = dr.groups * Sr; r1.lanes = 1;
  c1.splits = Sc; c1.groups = dc.groups * Sc; c1.lanes = 1;
  const ReduceJob s1r = {r1, 0u, RB_PTS, Sr > 1 ? RB_PART : RB_ROWCOL, 0, Sr > 1 ? part_r : rows};
  const ReduceJob s1c = {c1, 0u, RB_PTS, Sc > 1 ? RB_PART : RB_ROWCOL, 0, Sc > 1 ? part_c : cols};
  reduce_add_launch(rp, geom, num_cus, reduce_pair(s1r, s1c), one_lane ? SUMS_ON_FULL : SUMS_ON_PAIRS);
  SumDesc r2, c2;
  r2.mode = SUM_STRIDED; r2.groups = dr.groups; r2.count = Sr; r2.inner = dr.groups; r2.stride = 1; r2.istride = Sr; r2.group_shift = 0;
  c2 = r2; c2.groups = dc.groups; c2.count = Sc; c2.inner = dc.groups; c2.istride = Sc;
  ReduceJob s2r = reduce_job(geom, num_cus, RB_PART, part_r, RB_ROWCOL, rows, r2);
  ReduceJob s2c = reduce_job(geom, num_cus, RB_PART, part_c, RB_ROWCOL, cols, c2);
  if (Sr <= 1) s2r.d.groups = 0;
  if (Sc <= 1) s2c.d.groups = 0;
  reduce_add_launch(rp, geom, num_cus, reduce_pair(s2r, s2c), SUMS_ON_PAIRS);
}
// sum_idx (idx+1) B[idx] = sum_p 2^p U[p] + T, idx = hi*2^l + lo:
//   U[w][p], p < lo_bits from the column sums (weights lo), p >= lo_bits from the row sums (weights hi),
//   T[w] = plain sum of all buckets = sum of the row sums.
inline ReduceLaunch reduce_bit_sums(const MsmPlan &p, const BundleGeom &geom, int num_cus, u64 rows, u64 cols) {
  const u32 H = 1u << p.hi_bits, Lw = 1u << p.lo_bits, cb = p.c - 1;   // cb: bits of a bucket index
  SumDesc bl, bh_, bt;
  bl.mode = SUM_BITS; bl.stride = 1; bl.istride = 0;
  bl.groups = p.W * p.lo_bits; bl.count = Lw; bl.inner = std::max(1u, p.lo_bits); bl.group_shift = p.lo_bits;
  bh_ = bl; bh_.groups = p.W * p.hi_bits; bh_.count = H; bh_.inner = std::max(1u, p.hi_bits); bh_.group_shift = p.hi_bits;
  // the plain total is the sum of the column sums as well as of the row sums: take the shorter vector
  // (this job is the longest chain of the launch)
  const bool t_from_cols = Lw < H;
  bt.mode = SUM_STRIDED; bt.groups = p.W; bt.count = t_from_cols ? Lw : H; bt.inner = 1; bt.stride = 1; bt.istride = 0;
  bt.group_shift = t_from_cols ? p.lo_bits : p.hi_bits;
  ReduceLaunch l{};
  l.j[0] = reduce_job(geom, num_cus, RB_ROWCOL, cols, RB_BITS, 0, bl);
  l.j[1] = reduce_job(geom, num_cus, RB_ROWCOL, rows, RB_BITS, (u64)p.W * p.lo_bits, bh_);
  l.j[2] = reduce_job(geom, num_cus, RB_ROWCOL, t_from_cols ? cols : rows, RB_BITS, (u64)p.W * cb, bt);
  return l;
}
// rows (sum over lo, contiguous), columns (sum over hi, stride Lw), then bits.
// G workers per output chosen so that each launch is about one wavefront per SIMD.
inline ReducePlan reduce_plan(const MsmPlan &p, const BundleGeom &geom, int num_cus) {
  const bool G2 = geom.g2;
  const u32 H = 1u << p.hi_bits, Lw = 1u << p.lo_bits;
  ReducePlan rp{};
  // [r6] piece sums of the two-stage row / column sums (G1, 2^17 ... 2^21 buckets; below): pieces of `two_len` elements - the
  // launch of 2 NB / two_len lane pairs is then two wavefronts per SIMD (four with one lane per point and half the length)
  // [r6] the same for G2 sets reduced on lane triples (the 2^19 buckets of a 20-bit table): 16 workers per wavefront
  const bool TWO_STAGE_FR = geom.half_kind != WK_NONE;   // G1, and G2 in lane triples
  u32 two_len = 16;
  if (TWO_STAGE_FR) {
    const u64 target = (u64)num_cus * 4 * 2 * (G2 ? 16 : 32);
    two_len = 4;
    while (two_len < 64 && 2ull * p.NB / two_len > target) two_len <<= 1;
  }
  rp.two_len = two_len;
  rp.want_part = TWO_STAGE_FR && p.NB >= (1u << 17) && p.NB <= (1u << 21) && Lw >= 32 && H >= 32;
  rp.rowcol_elems = (u64)p.W * (H + Lw);
  rp.part_elems = rp.want_part ? (u64)p.W * ((u64)H * (Lw / std::min(two_len, Lw)) + (u64)Lw * (H / std::min(two_len, H))) : 0;
  rp.bits_elems = (u64)p.W * p.c;   // per window: (c-1) bit sums U[w][p], then W plain totals T[w]

  const u64 rows = 0, cols = (u64)p.W * H;   // inside rowcol
  SumDesc dr, dc;
  dr.mode = SUM_STRIDED; dr.groups = p.W * H; dr.count = Lw; dr.inner = H; dr.stride = 1; dr.istride = Lw; dr.group_shift = p.c - 1;
  dc = dr; dc.groups = p.W * Lw; dc.count = H; dc.inner = Lw; dc.stride = Lw; dc.istride = 1;
  if (rp.want_part) {   // (the sizes and groups that reduce in two stages)
    reduce_two_stage(rp, geom, num_cus, dr, dc, rows, cols);
  } else {
    ReduceLaunch l = reduce_pair(reduce_job(geom, num_cus, RB_PTS, 0, RB_ROWCOL, rows, dr), reduce_job(geom, num_cus, RB_PTS, 0, RB_ROWCOL, cols, dc));
    if (G2 && geom.lanes == 1) pick_lanes_jointly(num_cus, l.j[0].d, l.j[1].d);
    reduce_add_launch(rp, geom, num_cus, l);
  }
  reduce_add_launch(rp, geom, num_cus, reduce_bit_sums(p, geom, num_cus, rows, cols));
  return rp;
}

}  // namespace bh
