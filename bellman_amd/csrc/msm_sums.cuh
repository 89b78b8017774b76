// Stage 5 of a multiexp, device side: the half-point adders, the worker policies and the ONE sum kernel written over them
// (its launches are planned by reduce_plan of msm_stage_plans.hpp and issued by launch_reduce of msm_ec.cuh).
#pragma once
#include <type_traits>

#include "msm_stage_plans.hpp"
#include "msm_workers.cuh"

namespace bh {

// shuffle-based tree reduction of per-worker points over groups of G consecutive workers of one wavefront;
// `sub` = the worker's index inside its group
template <class F>
__device__ __forceinline__ void group_reduce_points(XYZZ<F> &acc, u32 G, u32 sub) {
  constexpr int NW = sizeof(XYZZ<F>) / 4;
  for (u32 off = G >> 1; off >= 1; off >>= 1) {
    XYZZ<F> o;
    u32 *dst = reinterpret_cast<u32 *>(&o);
    const u32 *srcw = reinterpret_cast<const u32 *>(&acc);
#pragma unroll
    for (int i = 0; i < NW; i++) dst[i] = __shfl_down(srcw[i], off * F::LANES);
    if (sub < off) {
      XYZZ<F> r;
      xyzz_add(r, acc, o);
      acc = r;
    }
  }
}

// ============================================================================================
// 5. reductions: the half-point adder, the worker policies, and ONE sum kernel written over them
// ============================================================================================
// 5a. A point split over an x side and a y side: G1 on lane PAIRS ("K2"), G2 on lane SEXTETS ("K6")
// A reduction launch of a small or medium job uses a fraction of the chip and is a chain of dependent point additions
// (~14 deep for 4096 buckets), each 8.2 K instructions = 20 us on a wavefront that has its SIMD to itself.  Lanes are free
// there, so a point is split over two neighbouring lanes - the even lane holds (X, ZZ), the odd lane (Y, ZZZ) - and the
// general addition add-2008-s runs as SEVEN lane-local product slots instead of fourteen products:
//     slot   x side                    y side
//      1     U1 = X1 ZZ2               S1 = Y1 ZZZ2
//      2     U2 = X2 ZZ1               S2 = Y2 ZZZ1            then  P = U2 - U1 | R = S2 - S1
//      3     PP = P^2                  RR = R^2                exchange: x gets RR, y gets PP
//      4     PPP = P PP                ZT = ZZZ1 ZZZ2          exchange: y gets PPP
//      5     Q = U1 PP                 S1P = S1 PPP            x: X3 = RR - PPP - 2Q, D = Q - X3; exchange: y gets D
//      6     T = ZZ1 ZZ2               ZZZ3 = ZT PPP
//      7     ZZ3 = T PP                Y3 = R D - S1P
// (three 12-word exchanges); an addition has about half the latency of the one-lane form, and a worker holds 24 words of
// state instead of 48.  The rare equal-points case falls back to the doubling of the full-point form, computed
// redundantly by both sides.  Only the reduction kernels use it, and only for launches that leave at least half of the
// SIMDs empty (msm_enqueue).
// The same split on top of the lane triples of K3 (fp2k3.cuh) [r6]: a G2 point is held by two neighbouring triples - the
// even triple (X, ZZ), the odd triple (Y, ZZZ), each an Fp2 element in (c0, c1, c0 + c1) form - and a slot is one
// lane-local Fp product.  A level of a merge tree costs ~20 us instead of the ~37 us of the lane-triple form: what the big
// bucket runs of boolean-heavy G2 queries and the medium runs of small window tables are made of (a 90 %-boolean G2
// query of 2^19 points: 14 levels, 0.58 ms in lane triples - profiles/r6_call5_*).  Eight workers per wavefront (48
// lanes: a power of two for the shuffle trees).
struct HalfPt {
  fp_t u, v;   // x side: X, ZZ    y side: Y, ZZZ
};
__device__ __forceinline__ fp_t half_sel(bool y, const fp_t &x_v, const fp_t &y_v) {
  fp_t r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = y ? y_v.l[i] : x_v.l[i];
  return r;
}
// What a half-point form is made of: the field bundle F of one side (XYZZ<F> is the full point of the doubling fallback),
// the records it reads (XYZZ<Mem>), and how a lane finds its worker, its side and the other side's values.
struct PairHalf {   // G1: the even lane of a pair is the x side, the odd lane the y side
  typedef FpOps F;
  typedef FpOps Mem;
  static constexpr u32 LANES = 2, PER_WAVE = 32;
  __device__ __forceinline__ static bool index(u32 &in_block) { in_block = threadIdx.x >> 1; return true; }
  __device__ __forceinline__ static u32 role() { return k3_lane() & 1u; }
  __device__ __forceinline__ static u32 side() { return role(); }
  __device__ __forceinline__ static fp_t swap(const fp_t &x) {   // the value held by the other lane of my pair (DPP quad_perm [1,0,3,2])
    fp_t r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = (u32)__builtin_amdgcn_update_dpp(0, (int)x.l[i], 0xB1, 0xf, 0xf, false);
    return r;
  }
  __device__ __forceinline__ static bool flag_from(bool mine, u32 want_side) {   // the predicate as the `want_side` lane of my pair sees it
    const u32 lane = k3_lane();
    const u64 m = __ballot(mine);
    return (m >> ((lane & ~1u) | want_side)) & 1;
  }
  __device__ __forceinline__ static void load(HalfPt &h, const XYZZ<FpOps> *p) {
    const bool odd = side();
    h.u = odd ? p->y : p->x;
    h.v = odd ? p->zzz : p->zz;
  }
  __device__ __forceinline__ static void store(XYZZ<FpOps> *p, const HalfPt &h) {
    if (side()) { p->y = h.u; p->zzz = h.v; } else { p->x = h.u; p->zz = h.v; }
  }
};
constexpr u32 K6_PER_WAVE = 8;
struct SextetHalf {   // G2: the even triple of a sextet is the x side, the odd triple the y side
  typedef Fp2K3Ops F;
  typedef Fp2Ops Mem;
  static constexpr u32 LANES = 6, PER_WAVE = K6_PER_WAVE;
  __device__ __forceinline__ static bool index(u32 &in_block) {
    const u32 t = (k3_lane() * 43u) >> 8;   // sextet inside the wavefront
    in_block = (threadIdx.x >> 6) * PER_WAVE + t;
    return t < PER_WAVE;
  }
  __device__ __forceinline__ static u32 role() { const u32 l = k3_lane(); return l - 6u * ((l * 43u) >> 8); }   // lane % 6
  __device__ __forceinline__ static u32 side() { return role() >= 3u ? 1u : 0u; }
  __device__ __forceinline__ static fp_t swap(const fp_t &x) {   // the same role's value in the other triple of my sextet (ds_bpermute by +-3 lanes)
    const int src = (int)k3_lane() + (side() ? -3 : 3);
    fp_t r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = (u32)__shfl((int)x.l[i], src);
    return r;
  }
  // the (triple-uniform) predicate as the `want_side` triple of my sextet sees it
  __device__ __forceinline__ static bool flag_from(bool mine, u32 want_side) {
    const u32 lane = k3_lane();
    const u64 m = __ballot(mine);
    return (m >> (lane - role() + 3u * want_side)) & 1;
  }
  __device__ __forceinline__ static void load(HalfPt &h, const XYZZ<Fp2Ops> *p) {
    const bool y = side();
    Fp2K3Ops::load(h.u, y ? &p->y : &p->x);
    Fp2K3Ops::load(h.v, y ? &p->zzz : &p->zz);
  }
  __device__ __forceinline__ static void store(XYZZ<Fp2Ops> *p, const HalfPt &h) {
    const bool y = side();
    Fp2K3Ops::store(y ? &p->y : &p->x, h.u);
    Fp2K3Ops::store(y ? &p->zzz : &p->zz, h.v);
  }
};
template <class P>
__device__ __forceinline__ bool half_is_identity(const HalfPt &h) { return P::flag_from(P::F::is_zero(h.v), 0u); }   // ZZ == 0
// r = a + b; r may alias a.  Every lane of a worker takes the same branches.
template <class P>
__device__ __forceinline__ void half_add(HalfPt &r, const HalfPt &a, const HalfPt &b) {
  typedef typename P::F F;
  const bool y = P::side();
  if (half_is_identity<P>(a)) { r = b; return; }
  if (half_is_identity<P>(b)) { r = a; return; }
  fp_t t1, t2, d;
  F::mul(t1, a.u, b.v);                     // U1 | S1
  F::mul(t2, b.u, a.v);                     // U2 | S2
  F::sub(d, t2, t1);                        // P | R
  const bool dz = F::is_zero(d);
  if (P::flag_from(dz, 0u)) {               // P == 0: the same x coordinate
    if (P::flag_from(dz, 1u)) {             // ... and R == 0: the same point - the full-point doubling, both sides redundantly
      XYZZ<F> full, dbl;
      const fp_t ou = P::swap(a.u), ov = P::swap(a.v);
      full.x = y ? ou : a.u; full.y = y ? a.u : ou;
      full.zz = y ? ov : a.v; full.zzz = y ? a.v : ov;
      xyzz_dbl(dbl, full);
      r.u = y ? dbl.y : dbl.x;
      r.v = y ? dbl.zzz : dbl.zz;
    } else {
      fe_zero(r.u); fe_zero(r.v);           // opposite points
    }
    return;
  }
  fp_t sq, m4, m5, m6, m7;
  F::sqr(sq, d);                            // PP | RR
  const fp_t osq = P::swap(sq);             // x side: RR    y side: PP
  const fp_t pp = y ? osq : sq;             // PP on both sides
  F::mul(m4, half_sel(y, d, a.v), half_sel(y, sq, b.v));        // P PP | ZZZ1 ZZZ2
  const fp_t om4 = P::swap(m4);
  const fp_t ppp = y ? om4 : m4;            // PPP on both sides
  F::mul(m5, t1, half_sel(y, pp, ppp));     // Q | S1P
  fp_t x3, dq, y3;
  F::sub(x3, osq, ppp);                     // x side: RR - PPP (the y side computes garbage it never uses)
  F::sub(x3, x3, m5);
  F::sub(x3, x3, m5);                       // X3 = RR - PPP - 2Q
  F::sub(dq, m5, x3);                       // Q - X3
  const fp_t odq = P::swap(dq);             // y side: Q - X3
  F::mul(m6, half_sel(y, a.v, m4), half_sel(y, b.v, ppp));      // T | ZZZ3
  F::mul(m7, half_sel(y, m6, d), half_sel(y, pp, odq));         // ZZ3 | R (Q - X3)
  F::sub(y3, m7, m5);                       // y side: Y3 = R (Q - X3) - S1P
  r.u = y ? y3 : x3;
  r.v = y ? m6 : m7;
}
// shuffle tree over groups of G consecutive workers of one wavefront (G a power of two <= PER_WAVE)
template <class P>
__device__ __forceinline__ void half_group_reduce(HalfPt &acc, u32 G, u32 sub) {
  for (u32 off = G >> 1; off >= 1; off >>= 1) {
    HalfPt o;
#pragma unroll
    for (int i = 0; i < 12; i++) {
      o.u.l[i] = __shfl_down(acc.u.l[i], off * P::LANES);
      o.v.l[i] = __shfl_down(acc.v.l[i], off * P::LANES);
    }
    if (sub < off) half_add<P>(acc, acc, o);   // the lanes of a worker take the branch together (sub is a property of the worker)
  }
}

// 5b. Worker policies: what the sum kernel and the merge kernels are written over.  A worker is a lane / lane pair / lane
// triple of bundle F holding an XYZZ point, or a lane pair (G1) / sextet (G2) holding half a point (5a).  PER_WAVE workers
// of a wavefront take part in shuffle trees; SOLO_PER_WAVE fit where every worker sums alone (all 21 lane triples).
template <class F>
struct XyzzWorker {
  typedef XYZZ<F> Pt;
  typedef F Ops;
  typedef typename F::Mem Mem;
  static constexpr u32 PER_WAVE = tree_per_wave<F>(), SOLO_PER_WAVE = default_per_wave<F>(), LANES = F::LANES;
  __device__ __forceinline__ static bool index(u32 &in_block, u32 per_wave = PER_WAVE) { u32 g; return worker_index<F>(per_wave, in_block, g); }
  __device__ __forceinline__ static u32 role() { return worker_role<F>(); }
  __device__ __forceinline__ static void identity(Pt &p) { xyzz_set_identity(p); }
  __device__ __forceinline__ static bool is_identity(const Pt &p) { return xyzz_is_identity(p); }
  __device__ __forceinline__ static void load(Pt &p, const XYZZ<Mem> *m) { load_xyzz<F>(p, m); }
  __device__ __forceinline__ static void store(XYZZ<Mem> *m, const Pt &p) { store_xyzz<F>(m, p); }
  __device__ __forceinline__ static void add(Pt &acc, const Pt &o) { Pt r; xyzz_add(r, acc, o); acc = r; }
  __device__ __forceinline__ static void tree(Pt &acc, u32 G, u32 sub) { group_reduce_points<F>(acc, G, sub); }
};
template <class P>
struct HalfWorker {
  typedef HalfPt Pt;
  typedef P Half;
  typedef typename P::Mem Mem;
  static constexpr u32 PER_WAVE = P::PER_WAVE, SOLO_PER_WAVE = P::PER_WAVE, LANES = P::LANES;
  __device__ __forceinline__ static bool index(u32 &in_block, u32 = PER_WAVE) { return P::index(in_block); }
  __device__ __forceinline__ static u32 role() { return P::role(); }
  __device__ __forceinline__ static void identity(Pt &p) { fe_zero(p.u); fe_zero(p.v); }
  __device__ __forceinline__ static bool is_identity(const Pt &p) { return half_is_identity<P>(p); }
  __device__ __forceinline__ static void load(Pt &p, const XYZZ<Mem> *m) { P::load(p, m); }
  __device__ __forceinline__ static void store(XYZZ<Mem> *m, const Pt &p) { P::store(m, p); }
  __device__ __forceinline__ static void add(Pt &acc, const Pt &o) { half_add<P>(acc, acc, o); }
  __device__ __forceinline__ static void tree(Pt &acc, u32 G, u32 sub) { half_group_reduce<P>(acc, G, sub); }
};
typedef HalfWorker<PairHalf> K2Worker;
typedef HalfWorker<SextetHalf> K6Worker;
// the id the host plans and the tests know a worker kind by (msm_stage_plans.hpp; the forms of bh_test_sum_jobs_dev)
template <class WK>
constexpr u32 worker_kind() {
  return std::is_same<WK, XyzzWorker<FpOps>>::value ? WK_XYZZ_FP : std::is_same<WK, K2Worker>::value ? WK_K2 :
         std::is_same<WK, XyzzWorker<Fp2Ops>>::value ? WK_XYZZ_FP2 : std::is_same<WK, XyzzWorker<Fp2K3Ops>>::value ? WK_XYZZ_FP2K3 :
         std::is_same<WK, XyzzWorker<Fp2PairOps>>::value ? WK_XYZZ_FP2PAIR : std::is_same<WK, K6Worker>::value ? WK_K6 : WK_NONE;
}
// A group of wpg * PW workers spans wpg wavefronts (a power of two): tree inside each wavefront, the partials through LDS,
// tree over the partials in the group's first wavefront -> the group's first worker.  `t` = worker inside the workgroup;
// every thread of the workgroup calls it.
template <class WK>
__device__ __forceinline__ void fold_over_waves(typename WK::Pt &acc, bool live, u32 PW, u32 wpg, u32 t, typename WK::Pt (*wave_part)[WK::LANES]) {
  const u32 wave = threadIdx.x >> 6, t_in_wave = t - wave * PW, role = WK::role();
  WK::tree(acc, PW, t_in_wave);
  if (live && t_in_wave == 0) wave_part[wave][role] = acc;
  __syncthreads();
  if ((wave & (wpg - 1)) == 0) {
    if (live && t_in_wave < wpg) acc = wave_part[wave + t_in_wave][role]; else WK::identity(acc);
    WK::tree(acc, wpg, t_in_wave);
  }
}

// 5c. The sum kernel: G workers per output point (serial partial sums, then a tree)
// the j-th index with bit k set, j = 0, 1, ...  (SUM_BITS walks exactly the selected half of its vector: striding over ALL
// indices left the workers whose own index has bit k clear - k < log2 G - with nothing to add and the others with twice the
// chain; [r6] 13 -> 9 levels for the bit sums of a 2^15-bucket window, 37 -> 21 for a 2^19-bucket set)
__device__ __forceinline__ u32 nth_with_bit(u32 j, u32 k) { return ((j >> k) << (k + 1)) | (1u << k) | (j & ((1u << k) - 1u)); }
// out[g] = sum of a set of in[] points chosen by the mode:
//   SUM_STRIDED: g = (outer, inner): elements in[(outer << group_shift) + inner*istride + t*stride], t < count
//   SUM_BITS   : g = (outer, k):     elements in[(outer << group_shift) + i], i < count, bit k of i set
template <class M>   // the records' field bundle
struct SumJob {
  const XYZZ<M> *in;
  XYZZ<M> *out;
  SumDesc d;       // (groups == 0: nothing to do)
  u32 nblocks = 0; // workgroups assigned to this job: sum_count fills it in
};
// up to three independent reductions per launch (rows + columns, then the bit-sum sets and the
// plain window totals): they are latency-bound, so sharing a launch lets the hardware overlap them.
template <class M>
struct SumJobs {
  SumJob<M> j[3];
};
// worker `sub` of the G that share output g adds up its share of the output's elements
template <class WK>
__device__ __forceinline__ void partial_sum(typename WK::Pt &acc, const SumDesc &d, const XYZZ<typename WK::Mem> *in, u32 g, u32 sub, u32 G) {
  const u32 gg = g / d.splits, len = d.count / d.splits, k0 = (g % d.splits) * len;   // (splits == 1: the whole group)
  const u32 outer = gg / d.inner, in_idx = gg % d.inner;
  const XYZZ<typename WK::Mem> *base = in + ((u64)outer << d.group_shift);
  if (d.mode == SUM_STRIDED) {
    for (u32 k = k0 + sub; k < k0 + len; k += G) {
      typename WK::Pt o;
      WK::load(o, base + (u64)in_idx * d.istride + (u64)k * d.stride);
      WK::add(acc, o);
    }
  } else {  // SUM_BITS: in_idx = bit position
    for (u32 j = sub; j < (d.count >> 1); j += G) {
      typename WK::Pt o;
      WK::load(o, base + nth_with_bit(j, in_idx));
      WK::add(acc, o);
    }
  }
}
// workers of a wavefront in a job of `lanes` workers per output: the rule of sum_workers_per_wave (msm_stage_plans.hpp), which
// the plans count with.  The kernel keeps its own expression over the worker's constants - written as a call of that function
// the lane-pair and lane-sextet kernels compile to other code (227 instead of 233 VGPRs on two wavefronts of lane pairs), which
// wants a measurement of its own - and sum_rule_agrees pins the two together
template <class WK>
BH_HD constexpr u32 sum_per_wave(u32 lanes) { return (WK::SOLO_PER_WAVE != WK::PER_WAVE && lanes == 1) ? WK::SOLO_PER_WAVE : WK::PER_WAVE; }
template <class WK>
constexpr bool sum_rule_agrees() {
  for (u32 lanes = 0; lanes <= 4 * 64; lanes++)   // every lane count a workgroup of up to four wavefronts can hold
    if (sum_per_wave<WK>(lanes) != sum_workers_per_wave(WK::PER_WAVE, WK::SOLO_PER_WAVE, lanes)) return false;
  return true;
}
static_assert(sum_rule_agrees<XyzzWorker<FpOps>>() && sum_rule_agrees<K2Worker>() && sum_rule_agrees<XyzzWorker<Fp2Ops>>() &&
              sum_rule_agrees<XyzzWorker<Fp2K3Ops>>() && sum_rule_agrees<K6Worker>(), "kernel and plans count a wavefront's workers alike");
// the one-lane and lane-triple forms put 64 workers in a workgroup: one wavefront of single lanes, or FOUR wavefronts of
// 16 lane triples - so that a K3 reduction can also put up to 64 workers on one output; with 16 the 256-element column
// sums of a window table's 2^15 buckets were 16 + 4 additions deep
template <class F>
constexpr u32 sum_waves() { return F::LANES == 3 ? 4u : 1u; }
// A workgroup is NWAVES wavefronts; a group of G <= PER_WAVE workers folds inside its wavefront, a wider one (up to the
// whole workgroup) through LDS.  What runs where (msm_enqueue decides):
//   one lane per point, 1 wavefront      G1 and single-lane G2 launches that fill the chip
//   lane triples, 4 wavefronts           the same for K3-form G2
//   lane pairs, 1 wavefront              G1 launches that leave SIMDs empty: 32 workers per workgroup
//   lane pairs, 2 or 4 wavefronts        ONE output per workgroup (G = 32 NWAVES) for the handful of long sums a big single
//                                        bucket set ends in (the 20-bit window table of a 2^20-point G1 query: 10 + 9 bit
//                                        sums and a total over 512 selected points each were 16 serial additions + 5 levels
//                                        on one wavefront; 2 + 5 + 3 here)
//   lane sextets, 4 wavefronts           G2 launches that leave the chip mostly empty (the bucket sets of small window
//                                        tables: a MiMC-322 proof's G2 job spent 2 x 136 us here in lane triples)
template <class WK, u32 NWAVES>
__global__ __launch_bounds__(64 * NWAVES, WK::LANES == 3 ? 2 : 1) void msm_sum_kernel(SumJobs<typename WK::Mem> jobs) {
  typedef typename WK::Pt Pt;
  u32 blk = blockIdx.x;
  u32 which = 0;
  if (blk >= jobs.j[0].nblocks) { blk -= jobs.j[0].nblocks; which = 1; if (blk >= jobs.j[1].nblocks) { blk -= jobs.j[1].nblocks; which = 2; } }
  const SumDesc d = jobs.j[which].d;
  const XYZZ<typename WK::Mem> *in = jobs.j[which].in;
  XYZZ<typename WK::Mem> *out = jobs.j[which].out;
  const u32 PW = sum_per_wave<WK>(d.lanes), WPB = PW * NWAVES;
  u32 t;
  const bool live = WK::index(t, PW);   // t = worker inside the workgroup
  const u32 G = d.lanes;
  const u32 g = (blk * WPB + t) / G;
  const u32 sub = t & (G - 1);
  // single-lane G2: partial sums live in LDS slots (an XYZZ<Fp2> accumulator is 96 VGPRs) and the tree reads
  // the partner's slot directly; every other form keeps registers + shuffles
  constexpr bool LDS_ACC = (WK::LANES == 1 && sizeof(Pt) > 200);
  __shared__ Pt lds_acc[LDS_ACC ? 64 : 1];
  __shared__ Pt wave_part[NWAVES][WK::LANES];
  Pt reg_acc;
  Pt &acc = LDS_ACC ? lds_acc[threadIdx.x] : reg_acc;
  WK::identity(acc);
  if (live && g < d.groups) partial_sum<WK>(acc, d, in, g, sub, G);
  if constexpr (LDS_ACC) {
    for (u32 off = G >> 1; off >= 1; off >>= 1) {
      __syncthreads();
      if (sub < off) WK::add(lds_acc[threadIdx.x], lds_acc[threadIdx.x + off]);
    }
  } else if (NWAVES == 1 || G <= PW) {
    WK::tree(acc, G, sub);
  } else {
    fold_over_waves<WK>(acc, live, PW, G / PW, t, wave_part);
  }
  if (live && sub == 0 && g < d.groups) WK::store(&out[g], acc);
}
// Clamps every job's workers per output to what a workgroup holds and fills in its workgroups, by the rule the plans count
// with (sum_job_blocks, msm_stage_plans.hpp); returns their total
template <class WK, u32 NWAVES>
static u32 sum_count(SumJobs<typename WK::Mem> &js) {
  u32 total = 0;
  for (int q = 0; q < 3; q++) total += js.j[q].nblocks = sum_job_blocks(js.j[q].d, WK::PER_WAVE, WK::SOLO_PER_WAVE, NWAVES);
  return total;
}
template <class WK, u32 NWAVES>
static bool sum_launch(SumJobs<typename WK::Mem> js, hipStream_t st) {
  const u32 total = sum_count<WK, NWAVES>(js);
  if (!total) return true;
  hipLaunchKernelGGL((msm_sum_kernel<WK, NWAVES>), dim3(total), dim3(64 * NWAVES), 0, st, js);
  return hipGetLastError() == hipSuccess;
}

// 5d. A workgroup of the long-run kernels (msm_merge.cuh): LONG_THREADS threads fold pieces of long_piece partials
constexpr u32 LONG_THREADS = 256;
template <class WK>
constexpr u32 long_workers() { return (LONG_THREADS / 64) * WK::PER_WAVE; }
template <class WK>
constexpr u32 long_piece() { return 2 * long_workers<WK>(); }   // partials per piece

// the half-point worker of the merge bundle FR: lane pairs in G1, lane sextets for G2 in lane triples; one-lane G2 has none
template <class FR>
struct MergeWorkers {
  static constexpr bool G1_PAIRS = std::is_same<FR, FpOps>::value, G2_SEXTETS = std::is_same<FR, Fp2K3Ops>::value;
  static constexpr bool PAIRS_POSSIBLE = G1_PAIRS || G2_SEXTETS;   // "pairs" below: the half-point worker of the group
  typedef typename std::conditional<G1_PAIRS, K2Worker, typename std::conditional<G2_SEXTETS, K6Worker, XyzzWorker<FR>>::type>::type HalfWK;
};
// What the host plans of stages 4 and 5 read from the bundle (msm_stage_plans.hpp): taken from the worker types, so that the
// plans count with the kernels' own numbers.  The big pieces run on HalfWK, which is the full worker where the group has no
// half-point worker
template <class FR>
constexpr BundleGeom bundle_geom() {
  typedef XyzzWorker<FR> FullWK;
  typedef typename MergeWorkers<FR>::HalfWK HalfWK;
  constexpr bool HALF = MergeWorkers<FR>::PAIRS_POSSIBLE;
  return BundleGeom{worker_kind<FullWK>(), FullWK::PER_WAVE, FullWK::SOLO_PER_WAVE, FR::LANES, sum_waves<FR>(),
                    HALF ? worker_kind<HalfWK>() : WK_NONE, HALF ? HalfWK::PER_WAVE : 0u, long_piece<HalfWK>(), FR::Mem::WORDS == 24};
}
// (the values the planners' comments and the tests' models speak of)
static_assert(bundle_geom<FpOps>().full_kind == WK_XYZZ_FP && bundle_geom<FpOps>().half_kind == WK_K2 &&
              bundle_geom<FpOps>().per_wave == XyzzWorker<FpOps>::PER_WAVE && bundle_geom<FpOps>().solo_per_wave == XyzzWorker<FpOps>::SOLO_PER_WAVE && bundle_geom<FpOps>().half_per_wave == K2Worker::PER_WAVE &&
              bundle_geom<FpOps>().sum_waves == sum_waves<FpOps>() && bundle_geom<FpOps>().long_piece == long_piece<K2Worker>() && !bundle_geom<FpOps>().g2,
              "G1: one lane per point, half points on lane pairs");
static_assert(bundle_geom<Fp2K3Ops>().full_kind == WK_XYZZ_FP2K3 && bundle_geom<Fp2K3Ops>().half_kind == WK_K6 &&
              bundle_geom<Fp2K3Ops>().per_wave == XyzzWorker<Fp2K3Ops>::PER_WAVE && bundle_geom<Fp2K3Ops>().solo_per_wave == XyzzWorker<Fp2K3Ops>::SOLO_PER_WAVE &&
              bundle_geom<Fp2K3Ops>().half_per_wave == K6Worker::PER_WAVE && bundle_geom<Fp2K3Ops>().sum_waves == sum_waves<Fp2K3Ops>() &&
              bundle_geom<Fp2K3Ops>().long_piece == long_piece<K6Worker>() && bundle_geom<Fp2K3Ops>().g2,
              "G2 in lane triples, half points on lane sextets");
static_assert(bundle_geom<Fp2Ops>().full_kind == WK_XYZZ_FP2 && bundle_geom<Fp2Ops>().half_kind == WK_NONE && bundle_geom<Fp2Ops>().half_per_wave == 0 &&
              bundle_geom<Fp2Ops>().sum_waves == sum_waves<Fp2Ops>() && bundle_geom<Fp2Ops>().long_piece == long_piece<XyzzWorker<Fp2Ops>>() && bundle_geom<Fp2Ops>().g2,
              "G2 with one lane per point: no half-point worker");

}  // namespace bh
