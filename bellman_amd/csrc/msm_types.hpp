// Shared declarations of the MSM pipeline (see msm.hip for the overview).
#pragma once
#include "common.hpp"

namespace bh {

struct ErrFlags {       // device-side status word block
  u32 eof;              // a dense entry found the base cursor at/after the end (multiexp.rs:55-61,74-80)
  u32 ident;            // an identity base was consumed (multiexp.rs:63-65)
  u32 ident_top;        // ... in the reference's top window, before the first EOF entry
  u32 nlong;            // number of (medium) bucket runs queued for the wavefront-parallel merge
  u32 nbig;             // runs long enough for the workgroup-parallel merge instead: counted here alone, not in nlong
  u32 npieces;          // ... and the workgroup-sized pieces they were cut into (msm_merge_tail_kernel)
  // what the job executed (bh_msm_wait_stats): mixed additions into a non-empty accumulator by the accumulate launch
  // (entries that OPEN a bucket or a chunk partial are copies, ec.cuh xyzz_madd), zero digits the sort moved to the front
  unsigned long long madds, zeros;
};

enum { SUM_STRIDED = 1, SUM_BITS = 2 };
struct SumDesc {
  u32 mode;
  u32 groups;      // number of outputs
  u32 count;       // elements per group
  u32 inner;       // groups per outer index
  u32 stride;      // element stride inside a group
  u32 group_shift; // log2 of the elements spanned by one outer index
  u32 istride;     // STRIDED: element offset between consecutive inner indices
  u32 lanes;       // G: lanes cooperating on one output (power of two <= 64)
  u32 splits = 1;  // STRIDED: every group is cut into `splits` equal pieces of count / splits consecutive elements, each an
                   // output of its own (out[group * splits + piece]); `groups` then counts the pieces
};
struct LongRun {   // a bucket run that spans more chunks than its owner lane folds itself
  u32 w, lane, d;  // window, first chunk (holds the run's tail partial), digit
  u32 last;        // last chunk with a head partial of the run
};
// A run too long for a handful of lanes (boolean-heavy witnesses put a quarter of the scalars into bucket 1 of window 0 -
// the reason the reference has Exponent::One, multiexp.rs:172-182,245-252): its partials are cut into pieces of one
// workgroup's worth, pieces [piece0, piece0 + npieces) of the job; the workgroup that finishes the run's last piece folds
// the piece results (`done` counts finished pieces).
struct BigRun {
  u32 w, lane, d, last;
  u32 piece0, npieces, done, pad;
};

// per-job plan overrides (bh_msm_opts): zero = tuned default
struct MsmOpts {
  u32 c = 0;        // window bits
  u32 chunk = 0;    // K
  u32 flags = 0;    // BH_MSM_*
  // a shard of a multi-context multiexp (bh_msm_sharded_async): the reference's window size follows the TOTAL
  // number of exponents (multiexp.rs:318-322), and the shard reports whether an identity base was consumed in that
  // top window even when it saw no EOF itself - the fold needs it for the error precedence
  u64 ref_n = 0;
  bool always_resolve_ident = false;
  // a many-job (bh_msm_many_*): `vectors` scalar vectors of the job's n scalars each over ONE base vector and density
  // map, vector v at scalars + v * scalar_stride bytes; 0 = an ordinary job
  u32 vectors = 0;
  u64 scalar_stride = 0;
};

struct MsmPlan {
  u32 n, c, W, nb, NB, lo_bits, hi_bits, num_tiles, sort_passes;
  u32 chunk;             // K: sorted entries per accumulation lane
  u32 chunks_per_window; // ceil(n / K)
  // digit stage: nd scalars x Wd digits.  Classic plan: nd == n, Wd == W, base_stride == 0.
  // Window-table plan (bases registered with their multiples 2^(c*j) P): all Wd digit columns feed
  // ONE bucket set, so the stages after the digits see a single window of n = nd*Wd entries (W == 1)
  // and a pair's base field addresses table row j: j*base_stride + base index.
  u32 nd, Wd;
  u64 base_stride;
  // Many-plan (make_many_plan): `vectors` scalar vectors share the job; vector v owns the windows_per_vector bucket sets
  // [v * windows_per_vector, (v + 1) * windows_per_vector) - Wd of them (classic flavour, one per digit column) or one
  // (table flavour).  Every other plan reads as one vector that owns all W sets.
  u32 vectors = 1, windows_per_vector = 0;   // (0: all W)
};
// "one bucket set" used to mean "window-table plan": the fused digit / sort stage (msm_stages.hip 2b) and the one-launch
// small path are for a single vector's single set only - a many-plan over a table has one set PER VECTOR
inline bool plan_fused_sort(const MsmPlan &p) { return p.W == 1 && p.vectors == 1; }
// what a job copies to its pinned result buffer: the 256-byte status slot, then W * c bit sums and totals (XYZZ records)
inline size_t job_result_bytes(const MsmPlan &p, size_t xyzz_bytes) { return 256 + (size_t)p.W * p.c * xyzz_bytes; }
// multiples 2^(c*j) P_i, j < W, stored row-major [j][i] (row 0 = the bases themselves)
struct WindowTable {
  u32 c, W;
  u64 stride;   // number of bases per row
};

// Where a job's base points come from.  A handle (handles.hpp bh_bases) has up to three sources; api_msm.hip snapshots them once
// per job, under the context's job_mu, and msm_pick_sources - the ONE place that holds these rules - says which of them
// each kernel of the job reads and at what stride.  Host only, no HIP calls (tests/test_msm_sources_cpu.py).
struct BaseView {
  const void *ptr = nullptr;   // null: the view is absent
  u32 stride = 0;              // bytes from one record to the next
};
struct MsmBases {
  BaseView dense;    // the registered vector: 96 (G1) / 192 (G2) bytes apart
  BaseView padded;   // G1: a copy of it 128 bytes apart (one cache line per gather), or absent
  BaseView table;    // window table, row-major [tab.W][tab.stride] records at its own stride (G1: 96 or 128), or absent
  WindowTable tab = {0, 0, 0};
  u64 n = 0;         // points in the vector
};
// how the accumulate launch of the job holds its running sum: the padded copy is gathered by the first form only
enum AccForm { ACC_ONE_LANE_REGISTERS = 0, ACC_ONE_LANE_LDS = 1, ACC_MULTI_LANE = 2 };
struct MsmSources {
  bool valid = false;       // false: a table laid out as no kernel reads it (only G1 tables may sit at a 128-byte stride)
  bool use_table = false;   // the window-table plan
  BaseView gather;          // what the bucket accumulation (and the small path) gathers from
  BaseView resolve;         // the view whose leading n records the error-resolution pass reads
  bool small_path = false;  // the source allows the one-launch small path: msm_small_fill_kernel indexes Affine<M> *
};
inline MsmSources msm_pick_sources(const MsmBases &b, const MsmOpts &opts, u64 n, int group, AccForm form) {
  const u32 rec = group == BH_G1 ? 96u : 192u;
  MsmSources s;
  s.valid = !b.table.ptr || b.table.stride == rec || (group == BH_G1 && b.table.stride == 128u);
  if (!s.valid) return s;
  // a window table is used when it exists, nobody forces another window size, and its row indices and the job's pair
  // positions fit their 31- and 32-bit fields
  s.use_table = b.table.ptr && !(opts.flags & BH_MSM_NO_TABLE) && (opts.c == 0 || opts.c == b.tab.c) &&
                (u64)b.tab.W * b.tab.stride < ((u64)1 << 31) && (u64)b.tab.W * n < ((u64)1 << 32);
  const bool padded = b.padded.ptr && group == BH_G1 && form == ACC_ONE_LANE_REGISTERS;
  s.gather = s.use_table ? b.table : padded ? b.padded : b.dense;
  s.resolve = s.use_table ? b.table : b.dense;   // (row 0 of a table is a snapshot of the bases)
  s.small_path = s.use_table && b.table.stride == rec;
  return s;
}

struct MsmJobImpl {
  Context *ctx = nullptr;
  int group = BH_G1;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  hipEvent_t ev_sorted = nullptr, ev_accum = nullptr;   // stage boundaries (profiling)
  MsmPlan plan;
  std::vector<void *> dev_allocs;     // returned to the pool on wait
  void *host_result = nullptr;        // pinned (owned by `res`): W*c XYZZ + ErrFlags
  size_t host_result_bytes = 0;
  JobResources res;
  bool timed = false;                 // stage events recorded (BH_MSM_STAGE_TIMES)
  int early_rc = BH_OK;               // immediate result (n == 0 etc.)
  bool trivial = false;
  // a job answered on the host at issue time (a handful of terms, api_msm.hip): the affine record to hand out
  bool has_result = false;
  alignas(16) unsigned char result[192];
  // inputs needed again by the (rare) error-resolution pass
  const void *scalars_dev = nullptr;
  const u64 *density_dev = nullptr;
  const u32 *word_prefix = nullptr;
  BaseView resolve_bases;            // MsmSources::resolve
  u64 skip = 0, n_bases = 0;
  int fmt = 0;
  ErrFlags *err_dev = nullptr;
  // completion state (msm.hip): whoever completes the job - its bh_msm_wait, or another issuing thread under
  // back-pressure - holds `mu` while it synchronises the stream and runs the host tail, and leaves the outcome here
  u64 ref_n = 0;                     // MsmOpts::ref_n
  bool always_resolve_ident = false;
  bool saw_eof = false, saw_ident = false, saw_ident_top = false;   // after completion
  // the stages after the sort of a job issued with BH_MSM_HOLD (until it is started): msm_after_sort over a copy of the
  // job's AfterSort (msm_ec.cuh), which names everything a held job keeps
  std::function<int(MsmJobImpl &)> resume;
  std::mutex mu;
  bool done = false;
  int done_rc = BH_OK;
  float done_ms[4] = {0, 0, 0, 0};
  u64 done_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // bh_msm_wait_stats
  alignas(16) unsigned char done_out[192];
  // many-job: one affine record per vector (msm_finish); the device flags are per job, so when either is set no record
  // is produced and the caller answers every vector by the single-vector path (many_fallback)
  std::vector<unsigned char> many_out;
  bool many_fallback = false;
};


// msm_stages.hip: curve-independent stages (signed digits, radix sort, zero-digit counts)
struct MsmBuffers {
  u64 *pairs_a, *pairs_b;
  u32 *counts, *scan_tmp, *zstart, *word_prefix;   // zstart[w] = #entries with digit 0 in window w
  ErrFlags *err;
};
MsmPlan make_plan(u64 n, unsigned forced_c, unsigned forced_chunk, bool g2);
MsmPlan make_table_plan(u64 n, const WindowTable &t, unsigned forced_chunk, bool g2, int num_cus);
// k scalar vectors of n scalars in one job: table != null -> table flavour (W = k sets of n * Wd entries), else classic
// (W = k * ceil(256 / c) sets of n entries, set v * Wc + w = digit w of vector v)
MsmPlan make_many_plan(u64 n, u64 k, const WindowTable *table, unsigned forced_c, unsigned forced_chunk, bool g2, int num_cus);
bool many_plan_valid(const MsmPlan &p, u64 n_bases);   // the 32-bit limits of the pipeline
unsigned table_window_bits(u64 n_bases, bool g2);   // the c a window table is built for by default
size_t scan_tmp_elems(u64 n);
size_t sort_counts_elems(const MsmPlan &p);   // MsmBuffers::counts holds this many + 1, scan_tmp scan_tmp_elems of that
// runs stages 1-2 (+ per-window first non-zero position) on `st`; *sorted_out = sorted pairs
// (scalar_stride: bytes between the scalar vectors of a many-plan)
int msm_run_stages(const MsmPlan &p, const MsmBuffers &b, const void *scalars_dev, int fmt, const u64 *density_dev,
                   u64 skip, u64 n_bases, hipStream_t st, const u64 **sorted_out, u64 scalar_stride = 0);

// msm_g1.hip / msm_g2.hip
int msm_enqueue_g1(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                   const u64 *density_dev, const MsmOpts &opts);
int msm_enqueue_g2(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                   const u64 *density_dev, const MsmOpts &opts);
int msm_finish_g1(MsmJobImpl &job, void *out_affine, float *ms);   // ms: float[4] or null
int msm_finish_g2(MsmJobImpl &job, void *out_affine, float *ms);
int fixed_base_mul_g1(const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev, hipStream_t st, void *table_dev);
int fixed_base_mul_g2(const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev, hipStream_t st, void *table_dev);
constexpr size_t FIXED_BASE_TABLE_RECORDS = 32 * 255;   // point_kernels.cuh FB_ROWS x FB_COLS

}  // namespace bh
