// Stage 4 of a multiexp, first half: bucket accumulation over equal chunks of the sorted stream, the one-launch small path,
// and the error-resolution pass (launched by launch_accumulate / msm_enqueue / msm_finish of msm_ec.cuh).
#pragma once
#include "msm_scalar.cuh"
#include "msm_stage_plans.hpp"
#include "msm_sums.cuh"

namespace bh {

// Only launched when both EOF and an identity were seen: decides which error the reference
// would report (the highest window's, i.e. the first failing element of the top window;
// multiexp.rs:295-300).  c_ref = reference window size, top window = bits [lo_ref, 256).
template <class F>
__global__ void msm_err_resolve_kernel(const void *scalars, int fmt, u32 n, const u64 *density,
                                       const u32 *word_prefix, u64 skip, u64 n_bases,
                                       const Affine<F> *bases, u32 base_stride, u32 lo_ref, ErrFlags *err) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u64 k = skip + i;
  if (density) {
    const u64 word = density[i >> 6];
    if (!((word >> (i & 63)) & 1)) return;
    k = skip + word_prefix[i >> 6] + __popcll(word & (((u64)1 << (i & 63)) - 1));
  }
  if (k >= n_bases) return;   // at/after the first EOF entry (k is monotone in i)
  fr_t s;
  load_scalar(scalars, i, fmt, s);
  bool top_nonzero = false;
  for (u32 b = lo_ref; b < 256; b += 16) top_nonzero |= extract_bits(s, b, (256 - b) < 16 ? (256 - b) : 16) != 0;
  if (!top_nonzero) return;
  // (the records the bucket accumulation of this job read: `base_stride` bytes apart)
  if (aff_is_identity(*reinterpret_cast<const Affine<F> *>(reinterpret_cast<const char *>(bases) + (size_t)k * base_stride)))
    atomicOr(&err->ident_top, 1u);
}

// ============================================================================================
// 4. bucket accumulation over equal chunks of the sorted stream
// ============================================================================================
// Lane l of window w owns sorted entries [z_w + l*K, z_w + (l+1)*K).  Buckets that lie completely
// inside the chunk are written straight to pts[bucket]; the (at most two) buckets shared with
// the neighbouring chunks go to head[l] / tail[l] and are folded by msm_merge_chunks_kernel.
struct ChunkView {
  u32 begin, end;       // entry range inside the window
  u32 d_first, d_last;  // digits of the first / last entry
  bool head_partial;    // first bucket started in an earlier chunk
  bool tail_partial;    // last bucket continues in the next chunk
};
// The plan's K is sized for n entries per window, but zero digits (z of them, sorted to the front) are skipped: sparse
// density maps - create_proof's b_g1 / b_g2 queries use about half of the aux variables - and small scalars leave a
// large part of the window empty, and with the plan's K the upper part of the launch would then have nothing to do
// (measured: the 2^19 dense entries of a 2^20-term G2 multiexp ran on HALF of the chip's lanes, 11 ms instead of 5.5).
// Every kernel that walks chunks therefore derives the window's effective chunk length from its zero count, so that
// the n - z live entries are spread over all chunks_per_window lanes again; never below 8 (or the plan's K if smaller)
// so that runs do not shatter into many partials.
__device__ __forceinline__ u32 effective_chunk(u32 n, u32 z, u32 chunks_per_window, u32 K) {
  const u32 live = n - z;
  u32 k = (u32)(((u64)live + chunks_per_window - 1) / chunks_per_window);
  const u32 floor_k = K < 8u ? K : 8u;
  if (k < floor_k) k = floor_k;
  return k < K ? k : K;
}
__device__ __forceinline__ bool chunk_view(const u64 *src, u32 n, u32 z, u32 lane, u32 K, ChunkView &v) {
  const u64 b = (u64)z + (u64)lane * K;
  if (b >= n) return false;
  v.begin = (u32)b;
  v.end = (u32)min((u64)n, b + K);
  v.d_first = (u32)(src[v.begin] >> 32);
  v.d_last = (u32)(src[v.end - 1] >> 32);
  // (never look below z: with one bucket set the sort drops the zero digits and what lies there is not an entry)
  v.head_partial = v.begin > z && (u32)(src[v.begin - 1] >> 32) == v.d_first;
  v.tail_partial = v.end < n && (u32)(src[v.end] >> 32) == v.d_last;
  return true;
}

// Trips: every wavefront runs as many trips as its longest lane has entries; an entry that OPENS a bucket or a chunk
// partial - 0.78 M of the 13.63 M entries of the 2^20-term plan - is a copy inside xyzz_madd while the other lanes add.
// Letting the lane go on to its next entry within the same trip (one addition per trip in every lane) was built and
// measured SLOWER, +0.04 ms alone and +0.05 ms on top of the sliced addition: nearly every trip has an opener in one of
// its 64 lanes, and the whole wavefront then waits for that lane's second pair of dependent loads (entry, then base) -
// profiles/accumulate_slices_and_openers.txt.  The loop is the plain one.
// LDS_ACC: the running bucket sum lives in the lane's LDS slot instead of 48/96 VGPRs - for G2 this
// is the difference between spilling at one wave per SIMD and fitting two.
// (measured and removed in round 6: a variant that reads one word of the NEXT entry's record right before the iteration's
// last, inline product, so that a window table too big for the Infinity Cache is gathered through the L2 - no difference, 2.88
// against 2.90 ms over a 2 GB table: profiles/r6_call28_touch.txt)
template <class F, bool LDS_ACC>
__global__ __launch_bounds__(128) void msm_accumulate_kernel(const u64 *pairs, const u32 *zstart,
                                                             const Affine<typename F::Mem> *bases,
                                                             XYZZ<typename F::Mem> *pts, XYZZ<typename F::Mem> *head,
                                                             XYZZ<typename F::Mem> *tail, u32 n, u32 c, u32 K,
                                                             u32 chunks_per_window, ErrFlags *err, u32 base_stride) {
  static_assert(!LDS_ACC || F::LANES == 1, "the LDS accumulator belongs to the single-lane kernels");
  static_assert(F::LANES == 1 || F::LANES == 2 || F::LANES == 3, "one lane, a lane pair or a lane triple per group element");
  const u32 w = blockIdx.y;
  u32 in_block, lane;
  if (!worker_index<F>(default_per_wave<F>(), in_block, lane)) return;
  const u64 *src = pairs + (u64)w * n;
  ChunkView v;
  const u32 z = zstart[w];
  K = effective_chunk(n, z, chunks_per_window, K);
  if (lane >= chunks_per_window || !chunk_view(src, n, z, lane, K, v)) return;
  XYZZ<typename F::Mem> *bucket = pts + ((u64)w << (c - 1)) - 1;   // bucket[d], d = |digit| in [1, 2^(c-1)]
  const u64 slot = (u64)w * chunks_per_window + lane;
  __shared__ XYZZ<F> lds_acc[LDS_ACC ? 128 : 1];
  XYZZ<F> reg_acc;
  XYZZ<F> &acc = LDS_ACC ? lds_acc[threadIdx.x] : reg_acc;
  xyzz_set_identity(acc);
  u32 cur = v.d_first;
  bool saw_identity = false;
  u32 adds = 0;   // additions into a non-empty accumulator (the rest of the chunk's entries are copies): bh_msm_wait_stats
  // Software pipeline (one lane per G2 point only: the kernels that fit two wavefronts per SIMD would lose the second
  // one to the extra live registers, and the second wavefront already covers their loads): the entry two steps
  // ahead and the base point one step ahead are loaded by `prefetch`, which xyzz_madd calls right before its last
  // (inline) product - the only stretch of an iteration without an out-of-line call, i.e. without a forced
  // s_waitcnt vmcnt(0) (ec.cuh).  With one resident wavefront per SIMD the two dependent loads of an iteration were
  // 21 % of the kernel's time (profiles/archive/r2_call8_pmc_g2_accumulate.json).
  constexpr bool PIPELINED = F::LANES == 1 && F::WORDS == 24;
  // the mixed addition over sliced operands (ec.cuh): the G1 kernel with its accumulator in registers, the one measured
  constexpr bool SLICED_MADD = has_sliced_products<F>::value && F::LANES == 1 && !LDS_ACC;
  // record `idx` of the vector the accumulation gathers from: every variant reads at the caller's record stride
  auto base_at = [&](u32 idx) {
    return reinterpret_cast<const Affine<typename F::Mem> *>(reinterpret_cast<const char *>(bases) + (size_t)idx * base_stride);
  };
  if constexpr (PIPELINED) {
    u64 e = src[v.begin];
    u64 e1 = v.begin + 1 < v.end ? src[v.begin + 1] : 0;
    Affine<F> q;
    load_affine<F>(q, base_at((u32)e & 0x7fffffffu));
    for (u32 p = v.begin; p < v.end; p++) {
      const u32 d = (u32)(e >> 32);
      if (d != cur) {   // bucket `cur` ends inside this chunk
        store_xyzz<F>((cur == v.d_first && v.head_partial) ? &head[slot] : &bucket[cur], acc);
        xyzz_set_identity(acc);
        cur = d;
      }
      Affine<F> qn = q;
      u64 e2 = 0;
      auto prefetch = [&]() {
        if (p + 1 < v.end) load_affine<F>(qn, base_at((u32)e1 & 0x7fffffffu));
        if (p + 2 < v.end) e2 = src[p + 2];
      };
      if (aff_is_identity(q)) {
        saw_identity = true;
        prefetch();
      } else {
        if ((u32)e >> 31) F::neg(q.y, q.y);   // negative digit: add -P
        adds += xyzz_madd(acc, q, prefetch) ? 1u : 0u;
      }
      q = qn;
      e = e1;
      e1 = e2;
    }
  } else {
    for (u32 p = v.begin; p < v.end; p++) {
      const u64 e = src[p];
      const u32 d = (u32)(e >> 32);
      if (d != cur) {   // bucket `cur` ends inside this chunk
        store_xyzz<F>((cur == v.d_first && v.head_partial) ? &head[slot] : &bucket[cur], acc);
        xyzz_set_identity(acc);
        cur = d;
      }
      Affine<F> q;
      load_affine<F>(q, base_at((u32)e & 0x7fffffffu));
      if (aff_is_identity(q)) { saw_identity = true; continue; }
      if ((u32)e >> 31) F::neg(q.y, q.y);   // negative digit: add -P
      if constexpr (SLICED_MADD) adds += xyzz_madd_sliced<F, true>(acc, q) ? 1u : 0u;   // G1 in registers: every value cut once, products inline
      else adds += xyzz_madd(acc, q) ? 1u : 0u;
    }
  }
  store_xyzz<F>((cur == v.d_first && v.head_partial) ? &head[slot] : v.tail_partial ? &tail[slot] : &bucket[cur], acc);
  if (saw_identity) atomicOr(&err->ident, 1u);
  // (one address for the whole launch: the compiler's atomic optimizer folds a wavefront's adds into one atomic)
  if (worker_role<F>() == 0) {
    atomicAdd(&err->madds, (unsigned long long)adds);
    if (lane == 0) atomicAdd(&err->zeros, (unsigned long long)z);
  }
}

// ============================================================================================
// 4'. small multiexps over bases with a window table: digits + bucket accumulation in ONE launch, no sort
// ============================================================================================
// create_proof on a small circuit (MiMC-322: multiexps of 322-1023 terms) is bound by the number of launches - a job
// was ~17 of them, ~8 us of host time each.  For up to SMALL_MAX_SCALARS scalars whose Wd digits all go to the one
// bucket set of a window table, every workgroup recodes ALL scalars into signed digits in its LDS (a few scalars per
// thread, redundantly per workgroup) and then each worker owns one bucket and scans the digit table for its entries:
// density prefix, digits, radix sort, zero count, accumulation and the three merge kernels become one launch.
// (profiles/archive/r3_call7_small_fused.txt)
// The SMALL_* constants, the dynamic LDS size (small_fill_lds_bytes) and the gate that keeps a job inside them
// (small_fill_plan) are host plan data: msm_stage_plans.hpp
template <class F>
__global__ __launch_bounds__(SMALL_THREADS) void msm_small_fill_kernel(const void *scalars, int fmt, u32 nd, const u64 *density,
                                                             u32 *word_prefix_out, u64 skip, u64 n_bases, u32 c, u32 Wd,
                                                             u64 base_stride, const Affine<typename F::Mem> *table,
                                                             XYZZ<typename F::Mem> *pts, ErrFlags *err) {
  extern __shared__ u32 small_lds[];
  const u32 n_entries = nd * Wd;
  u32 *kidx = small_lds;                                   // [nd] base index of scalar i, ~0u = contributes nothing
  short *dig = reinterpret_cast<short *>(small_lds + nd);  // [Wd][nd] signed digits
  u32 *cnt = small_lds + nd + ((n_entries * 2 + 3) >> 2);  // [SMALL_THREADS] entries seen per bucket of this workgroup
  unsigned short *lists = reinterpret_cast<unsigned short *>(cnt + SMALL_THREADS);   // [SMALL_THREADS][SMALL_LIST_CAP] entry ids
  const u32 nwords = (nd + 63) / 64;
  cnt[threadIdx.x] = 0;
  // (a) every workgroup recodes all scalars (a few per thread)
  for (u32 i = threadIdx.x; i < nd; i += blockDim.x) {
    bool dense = true;
    u64 k = skip + i;
    if (density) {
      const u64 word = density[i >> 6];
      dense = (word >> (i & 63)) & 1;
      u32 before = 0;
      for (u32 w = 0; w < (i >> 6); w++) before += (u32)__popcll(density[w]);   // <= 32 words
      k = skip + before + __popcll(word & (((u64)1 << (i & 63)) - 1));
    }
    bool live = dense;
    if (dense && k >= n_bases) {   // every dense entry checks EOF first, whatever its scalar (multiexp.rs:55-61,74-80)
      if (blockIdx.x == 0) atomicOr(&err->eof, 1u);
      live = false;
    }
    fr_t s;
    if (live) load_scalar(scalars, i, fmt, s);
    const u32 half = 1u << (c - 1);
    u32 carry = 0;
    for (u32 w = 0; w < Wd; w++) {
      u32 v = (live ? extract_bits(s, w * c, c) : 0) + carry;
      carry = 0;
      int d = (int)v;
      if (v > half) { d = (int)v - (int)(1u << c); carry = 1; }
      dig[w * nd + i] = (short)d;
    }
    kidx[i] = live ? (u32)k : 0xffffffffu;
  }
  if (blockIdx.x == 0 && density && word_prefix_out)   // the (rare) error-resolution pass wants the word prefix
    for (u32 t = threadIdx.x; t <= nwords; t += blockDim.x) {
      u32 before = 0;
      for (u32 w = 0; w < t && w < nwords; w++) before += (u32)__popcll(density[w]);
      word_prefix_out[t] = before;
    }
  __syncthreads();
  // (b) the entries of this workgroup's buckets, one list per bucket (order within a list does not matter)
  constexpr u32 PW = tree_per_wave<F>();                        // workers per wavefront (a power of two)
  const u32 wpb = workers_per_block<F>(SMALL_THREADS, PW);
  const u32 bpb = wpb / SMALL_LANES_PER_BUCKET;                 // buckets per workgroup
  const u32 bucket_lo = blockIdx.x * bpb;   // buckets [bucket_lo, bucket_lo + bpb), bucket index = |digit| - 1
  for (u32 e = threadIdx.x; e < n_entries; e += blockDim.x) {
    const int d = dig[e];
    if (d == 0) continue;
    const u32 bkt = (u32)(d < 0 ? -d : d) - 1;
    if (bkt < bucket_lo || bkt >= bucket_lo + bpb) continue;
    const u32 slot = atomicAdd(&cnt[bkt - bucket_lo], 1u);
    if (slot < SMALL_LIST_CAP) lists[(bkt - bucket_lo) * SMALL_LIST_CAP + slot] = (unsigned short)e;
  }
  __syncthreads();
  // (c) SMALL_LANES_PER_BUCKET workers per bucket: every worker adds every 4th entry of the list, then a shuffle tree.
  // (One worker per bucket made the launch as long as the FULLEST bucket of a wavefront - 12 entries where the average
  // is 5 - at 15 us per addition; the chip is nearly empty during these launches, so lanes are free.)
  u32 in_block, worker;
  const bool has_worker = worker_index<F>(PW, in_block, worker);
  const u32 nb = 1u << (c - 1);
  const u32 local = in_block / SMALL_LANES_PER_BUCKET, sub = in_block % SMALL_LANES_PER_BUCKET;
  const u32 bkt = bucket_lo + local;
  const bool active = has_worker && local < bpb && bkt < nb;
  const u32 total = active ? cnt[local] : 0;
  XYZZ<F> acc;
  xyzz_set_identity(acc);
  bool saw_identity = false;
  auto add_entry = [&](u32 e) {
    const u32 w = e / nd, i = e - w * nd;
    const u32 k = kidx[i];
    if (k == 0xffffffffu) return;   // (cannot happen: such scalars have all-zero digits)
    Affine<F> q;
    load_affine<F>(q, table + ((u64)w * base_stride + k));
    if (aff_is_identity(q)) { saw_identity = true; return; }
    if (dig[e] < 0) F::neg(q.y, q.y);
    xyzz_madd(acc, q);
  };
  if (total <= SMALL_LIST_CAP) {
    for (u32 t = sub; t < total; t += SMALL_LANES_PER_BUCKET) add_entry(lists[local * SMALL_LIST_CAP + t]);
  } else {
    // a bucket fuller than its list (many equal scalars - boolean witnesses put every 1 into bucket 1): scan the table
    const int bucket = (int)bkt + 1;
    u32 seen = 0;
    for (u32 e = 0; e < n_entries; e++) {
      const int d = dig[e];
      if (d == bucket || d == -bucket) {
        if (seen % SMALL_LANES_PER_BUCKET == sub) add_entry(e);
        seen++;
      }
    }
  }
  group_reduce_points<F>(acc, SMALL_LANES_PER_BUCKET, sub);   // every lane of the wavefront takes part in the shuffles
  if (active && sub == 0) store_xyzz<F>(&pts[bkt], acc);
  if (saw_identity) atomicOr(&err->ident, 1u);
}

}  // namespace bh
