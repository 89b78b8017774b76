/* libbellman_hip - C ABI of the MI355X (gfx950) implementation of bellman's Groth16
 * proving hot path.  Plain pointers and sizes only; no exceptions cross this boundary.
 *
 * The reference (zkcrypto/bellman @ 2024-08-07) has no FFI of its own: the boundary it
 * exposes is a set of generic Rust signatures.  Each entry point below names the reference
 * interface it replaces (file:line under /root/reference); INTEGRATION.md shows the Rust
 * `extern "C"` block + shim a maintainer would add behind those signatures.
 *
 * DATA FORMATS (identical to `bls12_381 0.8.0` in-memory values on a little-endian host)
 *   Fr element   32 B  4 x u64 little-endian limbs.  FFT/polynomial data is in MONTGOMERY
 *                      form (R = 2^256), exactly the bytes of a Rust `bls12_381::Scalar`.
 *   MSM scalar   32 B  either canonical little-endian (BH_SCALARS_CANONICAL - the bits of
 *                      `Exponent::Bits`, src/multiexp.rs:179; a value >= q, which the reference
 *                      cannot produce, is taken mod q) or Montgomery (BH_SCALARS_MONT -
 *                      a Rust `Scalar` as is; converted on the device).
 *   G1 affine    96 B  x | y, each 6 x u64 LE limbs, Montgomery form (R = 2^384).
 *   G2 affine   192 B  x.c0 | x.c1 | y.c0 | y.c1 (Fp2 = c0 + c1*u).
 *                      The point at infinity is the ALL-ZERO record ((0,0) is not on either
 *                      curve).  bh_bases_register_* can translate `infinity` flag bytes.
 *
 * ERROR CODES map 1:1 onto bellman::SynthesisError (src/lib.rs:303-319):
 */
#ifndef BELLMAN_HIP_H
#define BELLMAN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_OK 0
#define BH_ERR_UNEXPECTED_IDENTITY 1 /* SynthesisError::UnexpectedIdentity   src/multiexp.rs:63-65   */
#define BH_ERR_UNEXPECTED_EOF 2      /* SynthesisError::IoError(UnexpectedEof) src/multiexp.rs:55-61,74-80 */
#define BH_ERR_DEGREE_TOO_LARGE 3    /* SynthesisError::PolynomialDegreeTooLarge src/domain.rs:57-59 */
#define BH_ERR_UNCONSTRAINED_VARIABLE 5 /* SynthesisError::UnconstrainedVariable  groth16/src/generator.rs:464-470 */
#define BH_ERR_INVALID_POINT 6       /* io::ErrorKind::InvalidData "invalid G1" / "invalid G2" groth16/src/lib.rs:300-304,326-330 */
#define BH_ERR_POINT_AT_INFINITY 7   /* io::ErrorKind::InvalidData "point at infinity"         groth16/src/lib.rs:306-315,332-341 */
#define BH_ERR_INVALID_VERIFYING_KEY 8 /* VerificationError::InvalidVerifyingKey  src/lib.rs:353-358 */
#define BH_ERR_INVALID_PROOF 9       /* VerificationError::InvalidProof           src/lib.rs:353-358 */
#define BH_ERR_INVALID_TRANSCRIPT 10  /* bh_powers_of_tau_verify: a consistency equation of the transcript fails (no reference twin) */
#define BH_ERR_UNSATISFIABLE 11       /* SynthesisError::Unsatisfiable  src/lib.rs:310 */
#define BH_ERR_HIP (-1)              /* HIP runtime failure (message on stderr) */
#define BH_ERR_INVALID_ARG (-2)      /* the reference would panic (e.g. density length mismatch,
                                        src/multiexp.rs:324-329; length mismatch src/domain.rs:155,174) */
#define BH_ERR_NO_DEVICE (-3)        /* no gfx950 device / kernels unavailable: there is NO CPU fallback */

#define BH_SCALARS_CANONICAL 0
#define BH_SCALARS_MONT 1

#define BH_G1 1
#define BH_G2 2

typedef struct bh_ctx bh_ctx;         /* one per (process, GPU); thread-safe */
typedef struct bh_bases bh_bases;     /* device-resident, immutable base vector (the CRS queries) */
typedef struct bh_msm_job bh_msm_job; /* an MSM in flight == bellman's Waiter<Result<G,_>> */

/* ---- context: replaces multicore::Worker::new() (src/multicore.rs:24-27) ------------- */
int bh_ctx_create(int device, bh_ctx **out);
/* Waits for the device, then frees the context's pools, streams and tables.  Jobs must have been waited on.  Base
 * handles (bh_bases) may be released before or AFTER this call: a handle that outlives its context keeps its own
 * device memory until bh_bases_release and can no longer be used for a multiexp. */
void bh_ctx_destroy(bh_ctx *ctx);
/* Worker::log_num_threads analogue (src/multicore.rs:29-31): log2 of the CU count. */
uint32_t bh_ctx_log_num_cus(const bh_ctx *ctx);
const char *bh_version(void);
/* Process-level runtime settings, to be called BEFORE the process makes its first HIP call (the HIP runtime reads
 * them when it initialises): asks for 16 hardware queues (GPU_MAX_HW_QUEUES, unless the variable is already set) -
 * a proof keeps 6-7 job streams in flight and the runtime's default of 4 queues serialises them.  Returns 1 when no
 * HIP call had been made through this library yet, 0 when it is (probably) too late to take effect.  The library
 * never changes the environment on its own. */
int bh_runtime_configure(void);
/* Limits of a context (0 / (size_t)-1 = leave unchanged):
 *   max_jobs_in_flight  multiexps issued and not yet completed.  At the limit bh_msm_async* completes the OLDEST job
 *                       on the calling thread before issuing (its result is kept for its bh_msm_wait) - the analogue
 *                       of Worker::compute running a task inline once 4 x threads are pending
 *                       (src/multicore.rs:47-73).  Default: BELLMAN_HIP_MAX_JOBS, else from the device's memory.
 *   pool_cap_bytes      cap on the device memory the context's workspace pool holds (0 = none; BELLMAN_HIP_POOL_CAP_MB).
 *                       An allocation that does not fit first returns idle blocks to the driver, then completes jobs in
 *                       flight as above, and only fails (BH_ERR_HIP) when nothing is left to wait for.  The same
 *                       happens when hipMalloc itself fails.
 *   table_budget_bytes  total size of the window tables built AUTOMATICALLY at registration (bh_bases_register etc.;
 *                       default a quarter of the device's memory, BELLMAN_HIP_TABLE_BUDGET_MB); bh_ctx_trim drops them.
 *   fft_table_budget_bytes  total size of the cached per-size FFT tables (default an eighth of the device's memory,
 *                       BELLMAN_HIP_FFT_TABLE_BUDGET_MB).  From 2^12 to 2^24 points a domain size caches n-entry
 *                       twiddle / coset tables (32 bytes per entry; up to 4 tables at two passes, 6 at three: 0.5 GB at
 *                       2^22, 3.2 GB at 2^24); a size whose complete set exceeds the budget runs on its small two-level
 *                       tables instead (two products per factor, same results), and a table that does not fit beside
 *                       the others first drops the least recently used other sizes.  bh_ctx_trim drops them all. */
int bh_ctx_set_limits(bh_ctx *ctx, uint32_t max_jobs_in_flight, size_t pool_cap_bytes, size_t table_budget_bytes,
                      size_t fft_table_budget_bytes);
typedef struct {
  int32_t device;
  uint32_t num_cus;
  uint64_t hbm_bytes;
  uint32_t hw_queues_requested;            /* GPU_MAX_HW_QUEUES when the context was created (0 = unset: runtime default, 4) */
  uint32_t hw_queues_set_before_hip_init;  /* 1 = set before this library's first HIP call (bh_runtime_configure or the
                                              caller's environment): the request can have taken effect */
  uint32_t max_jobs_in_flight, jobs_in_flight;
  uint64_t pool_bytes_held, pool_bytes_idle, table_bytes, table_budget;
  uint64_t fft_table_bytes, fft_table_budget;   /* the cached per-size FFT tables (bh_ctx_set_limits) */
} bh_ctx_info_t;
int bh_ctx_info(bh_ctx *ctx, bh_ctx_info_t *info);

/* ---- raw device memory helpers (so callers can keep vectors resident in HBM) -------- */
int bh_dev_alloc(bh_ctx *ctx, size_t bytes, void **dev_ptr);
int bh_dev_free(bh_ctx *ctx, void *dev_ptr);
int bh_dev_upload(bh_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int bh_dev_download(bh_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
int bh_dev_zero(bh_ctx *ctx, void *dev_ptr, size_t bytes);   /* hipMemsetAsync(0) on the context stream */
/* caller-owned streams (opaque hipStream_t) so that independent proofs issued from different host
 * threads do not serialise on the context stream; the *_on variants enqueue and return */
int bh_stream_create(bh_ctx *ctx, void **stream);
/* high != 0: a stream of the device's highest priority - for short work on a proof's critical path (the h block, whose
 * result the H multiexp waits for) that must not queue behind another job's long-running kernels */
int bh_stream_create_priority(bh_ctx *ctx, int high, void **stream);
int bh_stream_destroy(bh_ctx *ctx, void *stream);
int bh_stream_synchronize(bh_ctx *ctx, void *stream);
int bh_dev_upload_on(bh_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes, void *stream);
int bh_dev_zero_on(bh_ctx *ctx, void *dev_ptr, size_t bytes, void *stream);
int bh_ctx_synchronize(bh_ctx *ctx);
/* Scheduling hint.  Bucket accumulations that fill the chip run one after the other in issue order (two of them side by
 * side take twice as long each and every job's latency-bound tail ends up at the end).  This call makes the NEXT such
 * accumulation - and through that chain every later one - start after everything enqueued on `stream` so far:
 * create_proof puts its h block (a short chain of FFT passes that would otherwise crawl behind the accumulations' long
 * workgroups, with the H multiexp waiting for it) in front of its multiexps' accumulations this way, while their digit
 * and sort stages still run beside it.  Results never depend on it. */
int bh_ctx_accumulations_after(bh_ctx *ctx, void *stream);
/* returns the context's idle cached device memory (recycled job workspaces, FFT twiddle tables) to the
 * driver; waits for the device to be idle first.  Purely a memory-footprint control; call it while no
 * other thread is inside a call on this context.  Unless a multiexp is in flight it also drops the window tables that
 * registration built automatically: results do not change, but such handles run the classic plan (slower for vectors
 * that had a table) until bh_bases_precompute is called on them - nothing rebuilds a dropped table by itself. */
int bh_ctx_trim(bh_ctx *ctx);

/* ---- EvaluationDomain (src/domain.rs) ------------------------------------------------
 * mode: 0 fft (:81-83)  1 ifft (:85-99)  2 coset_fft (:115-118)  3 icoset_fft (:120-125).
 * `data` holds 2^log_n Montgomery Fr (the padded `coeffs` of from_coeffs, :47-79), natural
 * order in and out, transformed in place.  log_n >= 32 -> BH_ERR_DEGREE_TOO_LARGE (:57-59). */
#define BH_FFT 0
#define BH_IFFT 1
#define BH_COSET_FFT 2
#define BH_ICOSET_FFT 3
int bh_fft_fr(bh_ctx *ctx, void *data_host, uint32_t log_n, int mode);
/* same on a device pointer, asynchronous on `stream` (a hipStream_t; NULL = context stream) */
int bh_fft_fr_dev(bh_ctx *ctx, void *data_dev, uint32_t log_n, int mode, void *stream);
/* The same transforms over k vectors in one call - `EvaluationDomain::{fft, ifft, coset_fft, icoset_fft}` (src/domain.rs:81-125)
 * on k domains of one size, as a batch prover's k h blocks issue them (groth16/src/prover.rs:221-240 once per proof).
 * Vector j lives at data + j * stride_bytes, holds 2^log_n Montgomery Fr and is transformed in place; what lies between two
 * vectors is neither read nor written.  Up to 2^10 points a workgroup transforms 2^(11 - log_n) vectors at once; above, one
 * launch per pass covers every (tile, vector).
 *   flags  BH_FFT_MANY_FORCE   batched launches wherever they are valid (every shape)
 *          BH_FFT_MANY_SINGLE  k single-vector transforms, exactly what k calls of bh_fft_fr_dev enqueue
 *          0                   batched where it was measured to win (profiles/fft_many_bench.json), single elsewhere
 *          The result is the same bytes on all three.
 *   _dev_on  enqueue only: `scratch_dev` = scratch_bytes of caller-owned workspace (may be NULL up to 2^11; at least one
 *          vector, 32 << log_n bytes, above), which like the data must stay valid until `stream` has drained.  A scratch of
 *          S vectors lets S vectors share each launch: k > S runs ceil(k / S) sub-batches one after the other.
 *   _dev   takes the scratch from the context's pool and waits for the stream before it returns, as bh_fft_fr_dev does.
 *   bh_fft_fr_many  k contiguous vectors on the HOST (stride = 32 << log_n).
 * log_n >= 32 -> BH_ERR_DEGREE_TOO_LARGE (:57-59), checked first.  BH_ERR_INVALID_ARG: a null ctx or data pointer, a mode
 * outside 0..3, a stride below 32 << log_n or not a multiple of 32, unknown flag bits (or both flags), log_n > 11 with the
 * scratch null or smaller than one vector.  k = 0 is BH_OK and launches nothing. */
#define BH_FFT_MANY_FORCE 1u
#define BH_FFT_MANY_SINGLE 2u
int bh_fft_fr_many_dev_on(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                          void *scratch_dev, size_t scratch_bytes, void *stream);
int bh_fft_fr_many_dev(bh_ctx *ctx, void *data_dev, size_t stride_bytes, size_t k, uint32_t log_n, int mode, unsigned flags,
                       void *stream);
int bh_fft_fr_many(bh_ctx *ctx, void *data_host, size_t k, uint32_t log_n, int mode);
/* pointwise domain ops on device vectors of n Montgomery Fr:
 *   mul_assign (:154-170)  sub_assign (:173-189)  divide_by_z_on_coset (:139-151, n = 2^log_n)
 *   distribute_powers(g) (:101-113; g = 32-byte Montgomery Fr on the HOST) */
int bh_fr_mul_assign_dev(bh_ctx *ctx, void *a_dev, const void *b_dev, size_t n, void *stream);
int bh_fr_sub_assign_dev(bh_ctx *ctx, void *a_dev, const void *b_dev, size_t n, void *stream);
int bh_fr_divide_by_z_on_coset_dev(bh_ctx *ctx, void *a_dev, uint32_t log_n, void *stream);
int bh_fr_distribute_powers_dev(bh_ctx *ctx, void *a_dev, size_t n, const void *g_host, void *stream);
/* EvaluationDomain<Fr, Point<G>> (src/domain.rs:192-229 with the methods of :21-190): the same operations on device
 * vectors of affine G1 / G2 records (group = BH_G1 / BH_G2; Montgomery, identity = all-zero record), in place on `stream`
 * (NULL = context stream).  The ifft of [tau^i]G from a powers-of-tau transcript gives the Lagrange-basis points
 * [L_j(tau)]G.  Scalars and g_host are Montgomery Fr as above.  The points are NOT validated (a Point<G> holds a group
 * element by type): records that are not on the curve give meaningless records.  bh_fft_point_dev and
 * bh_point_distribute_powers_dev take pool workspace and wait for the stream before they return; the other three only
 * enqueue.  log_n >= 32 -> BH_ERR_DEGREE_TOO_LARGE, a bad group or mode -> BH_ERR_INVALID_ARG, n = 0 does nothing. */
int bh_fft_point_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, int mode, void *stream);   /* BH_FFT..BH_ICOSET_FFT */
int bh_point_distribute_powers_dev(bh_ctx *ctx, int group, void *points_dev, size_t n, const void *g_host, void *stream);
int bh_point_divide_by_z_on_coset_dev(bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, void *stream);
int bh_point_mul_assign_dev(bh_ctx *ctx, int group, void *points_dev, const void *scalars_dev, size_t n, void *stream);
int bh_point_sub_assign_dev(bh_ctx *ctx, int group, void *a_dev, const void *b_dev, size_t n, void *stream);
/* The whole h-polynomial block of create_proof (groth16/src/prover.rs:221-240), fused:
 * a,b,c = n_evals constraint evaluations each (Montgomery Fr, HOST); writes the m-1 quotient
 * coefficients (m = next pow2 >= n_evals, :238-239) to h_out_host (Montgomery) and returns
 * m-1 in *h_len.  Runs ifft/coset_fft x3, (a*b-c)/Z in one pass, icoset_fft. */
int bh_h_poly_fr(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host,
                 size_t n_evals, void *h_out_host, size_t *h_len);
/* device-resident variant: a,b,c are 2^log_n-element device vectors (clobbered); result in a */
int bh_h_poly_fr_dev(bh_ctx *ctx, void *a_dev, void *b_dev, void *c_dev, uint32_t log_n, void *stream);
/* the same, enqueue only (no synchronisation): `scratch_dev` = 2^log_n Fr of caller-owned workspace (may be NULL
 * up to 2^11), which like a, b, c must stay valid until `stream` has drained */
int bh_h_poly_fr_dev_on(bh_ctx *ctx, void *a_dev, void *b_dev, void *c_dev, void *scratch_dev, uint32_t log_n,
                        void *stream);
/* k h blocks in one call (groth16/src/prover.rs:221-240 for each of k proofs of one circuit): a_j, b_j, c_j at
 * base + j * stride_bytes.  For every j, a_j ends exactly as bh_h_poly_fr_dev_on leaves it (all 2^log_n words; the first
 * m - 1 are the h coefficients, :238-239); b_j and c_j are clobbered.  Seven batched transforms and one batched
 * (a*b-c)/Z pass (src/domain.rs:139-189).  Flags, scratch and return codes as bh_fft_fr_many_dev_on (a, b, c non-null). */
int bh_h_poly_fr_many_dev_on(bh_ctx *ctx, void *a_dev, void *b_dev, void *c_dev, size_t stride_bytes, size_t k, uint32_t log_n,
                             unsigned flags, void *scratch_dev, size_t scratch_bytes, void *stream);

/* ---- bases: the `(Arc<Vec<G::Affine>>, usize)` SourceBuilder (src/multiexp.rs:45-86) --
 * Uploads `n` affine points once (the CRS is immutable and shared by every proof,
 * groth16/src/lib.rs:443-473).  `stride` bytes between records; coordinates (Montgomery) at
 * byte offset 0; if inf_offset >= 0 the byte at that offset != 0 marks the identity
 * (the `infinity: Choice` of bls12_381's G1Affine/G2Affine), else identity == all-zero. */
int bh_bases_register(bh_ctx *ctx, int group, const void *host_points, size_t n, size_t stride,
                      long inf_offset, bh_bases **out);
/* Same, straight from bellman's serialized CRS (`Parameters::write`, groth16/src/lib.rs:258-287):
 * `n` uncompressed points in the Zcash encoding (`to_uncompressed()`: big-endian canonical
 * coordinates, 96 B for G1 = x|y, 192 B for G2 = x.c1|x.c0|y.c1|y.c0, flag bits in the top of byte
 * 0; the infinity flag yields the identity).  Byte order, flags and the conversion to Montgomery form
 * are handled on the device.  Like `from_uncompressed_unchecked` (lib.rs:296-300) no on-curve or
 * subgroup check is made; a compressed-form flag returns BH_ERR_INVALID_ARG. */
int bh_bases_register_uncompressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n,
                                   bh_bases **out);
/* `from_uncompressed` / `from_uncompressed_unchecked` + the identity test of Parameters::read
 * (groth16/src/lib.rs:289-341) for `n` uncompressed points, all on the device.  Without flags only
 * the encoding rules are enforced (flag bits, coordinates < p, a clean infinity encoding);
 * BH_POINTS_CHECKED adds the on-curve and prime-order-subgroup tests, BH_POINTS_FORBID_IDENTITY the
 * "point at infinity" rule.  On BH_ERR_INVALID_POINT / BH_ERR_POINT_AT_INFINITY *bad_index (optional)
 * is the first offending point in stream order, which is the one the reference reports. */
#define BH_POINTS_CHECKED 1u
#define BH_POINTS_FORBID_IDENTITY 2u
int bh_bases_read_uncompressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n, unsigned flags,
                               bh_bases **out, size_t *bad_index);
/* `from_compressed` / `from_compressed_unchecked` for `n` COMPRESSED points (48 B for G1, 96 B for G2 = x.c1|x.c0; byte 0
 * carries the flags compressed 0x80, infinity 0x40, sort 0x20), all on the device: the twin of bh_bases_read_uncompressed,
 * with the same flags, return codes and "first offending point in stream order" rule.  A point is valid iff the compressed
 * flag is set, every coordinate is < p, and either the infinity flag is set with every other bit clear (the identity) or
 * x^3 + b is a square - y is then the root whose "lexicographically largest" equals the sort flag.  BH_POINTS_CHECKED adds
 * the prime-order-subgroup test (by endomorphism: csrc/point_read.hip); without it the call is from_compressed_unchecked. */
int bh_bases_read_compressed(bh_ctx *ctx, int group, const void *host_bytes, size_t n, unsigned flags,
                             bh_bases **out, size_t *bad_index);
/* The same tests for records that are ALREADY RESIDENT: [first, first + count) of any handle - one made by
 * bh_bases_copy_dev / bh_bases_wrap_dev, by a point transform or a contribution step included.  flags as above: without
 * BH_POINTS_CHECKED only the identity rule (BH_POINTS_FORBID_IDENTITY) is applied; with it every record that is not the
 * identity (the all-zero record) must hold coordinates < p, satisfy y^2 = x^3 + b and lie in the prime-order subgroup - by
 * endomorphism (csrc/point_read.hip: two multiplications by the 64-bit |z| for G1, one for G2) instead of the [q] P test
 * of bh_bases_read_uncompressed.  Returns BH_OK, BH_ERR_INVALID_POINT or BH_ERR_POINT_AT_INFINITY; *bad_index (optional)
 * is the first offending record in order, relative to `first` - the rule of the readers.  status_host (optional, `count`
 * words, written for every record whatever the return code) receives the PointStatus bits of csrc/msm_types.hpp:
 * 0x04 a coordinate >= p, 0x10 identity, 0x20 off the curve, 0x40 not in the subgroup.  A range beyond the handle is
 * BH_ERR_INVALID_ARG, count = 0 is BH_OK.  Runs in chunks of 2^20 records (4 MB of status workspace) on a stream of its
 * own: thread-safe.  A wrapped handle is read as it is when the call runs. */
int bh_bases_validate(bh_ctx *ctx, const bh_bases *b, size_t first, size_t count, unsigned flags, uint32_t *status_host,
                      size_t *bad_index);
/* copies `count` device-resident affine records (Montgomery) starting at `first` back to the host */
int bh_bases_download(bh_ctx *ctx, const bh_bases *b, size_t first, size_t count, void *out_host);
/* the same range in the uncompressed encoding Parameters::write emits (groth16/src/lib.rs:258-287; 96 / 192 bytes per
 * point, big-endian coordinates, G2 c1 before c0, identity = flag byte 0x40): encoded on the device, count * 96|192 bytes
 * to out_host_bytes - the inverse of bh_bases_read_uncompressed */
int bh_bases_write_uncompressed(bh_ctx *ctx, const bh_bases *bases, size_t first, size_t count, void *out_host_bytes);
/* Window table for a registered base vector (optional; the CRS is fixed across proofs, groth16/src/lib.rs
 * :443-473 hands out the same Arc<Vec<Affine>> every time): stores 2^(c*j) P_i for every window j next to
 * the bases (W = ceil(256/c) rows, W x the memory).  Multiexps over such bases send every digit of a
 * scalar to ONE bucket set - one bucket reduction instead of W and no doubling chain over windows.
 * The result of a multiexp is the same group element either way.  window_bits = 0 picks the tuned
 * value for the vector length.  Registration (bh_bases_register / _uncompressed / bh_bases_copy_dev) builds this
 * table by itself for G1 vectors of up to 2^24 points and G2 vectors of up to 2^22 while the context's table
 * budget lasts (bh_ctx_set_limits): G1 vectors from 2^19 points take 20-bit rows - 13 rows, so a multiexp
 * performs 13 n additions instead of the 16 n of the classic 16-window plan - at 13 x 128 bytes per point (1.7 GB
 * per 2^20 points; built in ~0.13 s); G2 vectors keep 16-bit rows (20-bit ones on request: faster on uniform
 * scalars from 2^20 points, slower on boolean-heavy ones - their 2^19 buckets cost ~2 ms to reduce).  BH_ERR_HIP when the table does not fit in HBM (the handle stays usable
 * without it); BH_ERR_INVALID_ARG when W x n >= 2^31. */
int bh_bases_precompute(bh_ctx *ctx, bh_bases *b, unsigned window_bits);
int bh_bases_table_info(const bh_bases *b, unsigned *window_bits, unsigned *rows, size_t *bytes);
/* a new owned handle holding a device-to-device copy of `n` packed records */
int bh_bases_copy_dev(bh_ctx *ctx, int group, const void *dev_points, size_t n, bh_bases **out);
/* the device twin of bh_bases_download: copies records [first, first + count) of a handle into the caller's device buffer,
 * enqueued on `stream` (NULL = context stream).  `group` is the group the caller expects: a handle of the other group, or
 * a range beyond the handle's length, returns BH_ERR_INVALID_ARG (count = 0 only makes these checks). */
int bh_bases_copy_out_dev(bh_ctx *ctx, const bh_bases *b, int group, size_t first, size_t count, void *dst_dev, void *stream);
/* wrap an existing device array of packed 96/192-byte records (not owned): a LIVE view - nothing is copied or
 * precomputed from the buffer at wrap time (no host mirror for tiny multiexps, no automatic window table), every
 * multiexp reads the buffer as it is when the job runs; the caller orders its writes before issuing.
 * bh_bases_precompute on such a handle is an explicit SNAPSHOT of the buffer's contents at that call.  A multiexp
 * that does not use that table (BH_MSM_NO_TABLE, another window_bits) reads the live buffer, never the snapshot. */
int bh_bases_wrap_dev(bh_ctx *ctx, int group, const void *dev_points, size_t n, bh_bases **out);
void bh_bases_release(bh_ctx *ctx, bh_bases *b);
size_t bh_bases_len(const bh_bases *b);

/* ---- multiexp (src/multiexp.rs:305-332) ---------------------------------------------
 * Computes  sum_i [density_i] s_i * B[skip + rank_i]   (rank_i = #dense entries before i),
 * i.e. multiexp(pool, (bases, skip), density_map, exponents):
 *   scalars        n_scalars x 32 B (HOST unless *_dev), format per scalar_fmt
 *   density_words  NULL = FullDensity (:95-115); else LSB0 bitmap, ceil(n/64) u64 words
 *                  (DensityTracker's BitVec<usize,Lsb0>, :117-131); density_len must equal
 *                  n_scalars or BH_ERR_INVALID_ARG is returned (the reference panics, :324-329)
 * Returns immediately with a job (the Waiter); bh_msm_wait blocks (Waiter::wait,
 * src/multicore.rs:100-109), writes the AFFINE result record (96/192 B, Montgomery; all-zero =
 * identity) and returns BH_OK / BH_ERR_UNEXPECTED_IDENTITY / BH_ERR_UNEXPECTED_EOF with the
 * reference's precedence (highest failing window wins, :295-300).  Many jobs may be in
 * flight per context (create_proof issues 8, groth16/src/prover.rs:244-318). */
int bh_msm_async(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host,
                 size_t n_scalars, int scalar_fmt, const uint64_t *density_words,
                 size_t density_len, bh_msm_job **job);
int bh_msm_async_dev(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev,
                     size_t n_scalars, int scalar_fmt, const uint64_t *density_words_dev,
                     size_t density_len, bh_msm_job **job);
int bh_msm_wait(bh_msm_job *job, void *out_affine);
/* device time of the job's kernels in milliseconds (hipEvents on the job's stream; needs BH_MSM_STAGE_TIMES) */
int bh_msm_wait_timed(bh_msm_job *job, void *out_affine, float *device_ms);
/* as above with per-stage device times (hipEvents on the job's stream), milliseconds:
 * [0] whole pipeline  [1] digits + radix sort + task list  [2] bucket accumulation  [3] reductions;
 * zeros unless the job was issued with BH_MSM_STAGE_TIMES in bh_msm_opts.flags */
int bh_msm_wait_profile(bh_msm_job *job, void *out_affine, float *stage_ms4);
/* ... and with what the job EXECUTED, counted on the device (every job; no flag needed):
 * [0] sorted (digit, base) entries = windows x terms   [1] zero digits among them (skipped after the sort)
 * [2] mixed additions the accumulate launch performed into a non-empty accumulator - the entries that open a bucket or a
 *     chunk partial are copies (src/multiexp.rs:256-258 adds into an identity bucket likewise)
 * [3] chunk lanes of the accumulate launch   [4] window bits c   [5] chunk length K   [6] bucket sets W (1 = window-table
 * plan)   [7] digit columns per scalar.  What bench.py's roofline.alu and its check of the PMC files are computed from. */
int bh_msm_wait_stats(bh_msm_job *job, void *out_affine, float *stage_ms4, uint64_t *stats8);
/* The plan a multiexp of n terms over unregistered bases would run (host only, no context): out9 = c, windows, buckets
 * per window, K, chunks per window, sort passes, lo bits, hi bits of the two-dimensional bucket reduction, low 32 bits of
 * windows x n.  forced_c = 0: the tuned window size. */
int bh_msm_plan_info(size_t n, int group, unsigned forced_c, unsigned *out9);
/* Verification aid: runs the digit and sort stages of a G1 multiexp for window size c on n host scalars (src/multiexp.rs:
 * 159-208, 281-286: Exponent, chunks) and copies the sorted (|digit| << 32 | sign << 31 | index) pairs [windows * n] and
 * the per-window number of zero digits [windows] to the host. */
int bh_msm_debug_stages(bh_ctx *ctx, const void *scalars_host, size_t n, int scalar_fmt, unsigned c,
                        uint64_t *pairs_out_host, uint32_t *zstart_out_host);
/* r[i] = a[i] + b[i] for affine records on the HOST - used to fold the per-GPU partial results of
 * a base-sharded MSM after the all-gather, and g_a/g_b/g_c in create_proof. */
void bh_point_add(int group, void *r, const void *a, const void *b, size_t n);
/* r = [k] a on the HOST, k = 32-byte canonical little-endian scalar: the five single scalar
 * multiplications of create_proof (groth16/src/prover.rs:326-338, 342, 351) */
void bh_point_mul(int group, void *r, const void *a, const void *k_canonical);
/* r = sum_i [k_i] points[i] on the HOST (n affine records, n x 32-byte canonical scalars; scalars = NULL: all ones) with
 * one shared doubling chain and one inversion: g_c = ... + [s] a_answer + [r] b1_answer + h + l of create_proof
 * (groth16/src/prover.rs:339-354) in one call */
void bh_point_lincomb(int group, void *r, const void *points, const void *scalars_canonical, size_t n);
/* Per-job plan overrides (experiments, tests, tuning sweeps): NULL or all-zero = the tuned defaults.
 * They travel with the job, so concurrent jobs on one context never see each other's settings.  The
 * result is the same group element whatever the plan. */
typedef struct {
  uint32_t window_bits; /* c, 2..24; 0 = automatic */
  uint32_t chunk;       /* K: sorted entries per accumulation lane; 0 = automatic */
  uint32_t flags;       /* BH_MSM_* below */
} bh_msm_opts;
#define BH_MSM_ACC_REGISTERS 1u /* keep the running bucket sum in registers */
#define BH_MSM_ACC_LDS 2u       /* ... in LDS */
#define BH_MSM_NO_TABLE 4u      /* ignore a window table attached to the bases */
#define BH_MSM_NO_SMALL_PATH 8u /* run the full pipeline even for a handful of terms */
#define BH_MSM_STAGE_TIMES 64u  /* record the per-stage HIP events bh_msm_wait_profile reports (4 extra API calls) */
#define BH_MSM_HOLD 128u        /* enqueue only the digit / sort stage; bh_msm_start (or the job's wait) enqueues the rest */
#define BH_MSM_G2_SINGLE_LANE 16u /* G2: force the one-lane-per-point kernels (default: merge + reduction above 2^17 buckets) */
#define BH_MSM_G2_LANE_TRIPLES 32u /* G2: force the lane-triple (Karatsuba) kernels (default below 2^15 terms) */
#define BH_MSM_G2_LANE_PAIRS 256u /* G2: force the lane-pair kernel for the bucket accumulation (default from 2^15 terms) */
int bh_msm_async_opts(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host,
                      size_t n_scalars, int scalar_fmt, const uint64_t *density_words,
                      size_t density_len, const bh_msm_opts *opts, bh_msm_job **job);
int bh_msm_async_dev_opts(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev,
                          size_t n_scalars, int scalar_fmt, const uint64_t *density_words_dev,
                          size_t density_len, const bh_msm_opts *opts, bh_msm_job **job);
/* Two-phase issue (scheduling only; results never depend on it): a job issued with BH_MSM_HOLD enqueues its digit and
 * sort stages and stops; bh_msm_start enqueues bucket accumulation, reductions and the result copy.  Chip-filling
 * accumulations run in the order they are started, and the first one started waits for the sort stages of every held
 * job issued before it: create_proof issues its multiexps held and starts them longest first, so that no sort runs
 * beside an accumulation.  bh_msm_wait on a job that was never started starts it. */
int bh_msm_start(bh_msm_job *job);

/* as bh_msm_async_dev_opts, with the job ORDERED AFTER everything enqueued so far on `after_stream` (a stream of
 * bh_stream_create, or any hipStream_t of this device): the scalars may still be being produced there - create_proof's
 * H multiexp consumes the h block's coefficients (groth16/src/prover.rs:221-245) without the host waiting in between */
int bh_msm_async_dev_after(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t n_scalars,
                           int scalar_fmt, const uint64_t *density_words_dev, size_t density_len, const bh_msm_opts *opts,
                           void *after_stream, bh_msm_job **job);

/* ---- several scalar vectors over ONE base vector in one job ---------------------------------------------
 * out[v] = multiexp(pool, (bases, skip), density, exponents_v) for v < k: one base vector, one density map (it belongs
 * to the circuit), k scalar vectors of n_scalars x 32 bytes, vector v at scalars + v * stride_bytes (stride_bytes >=
 * 32 n_scalars and a multiple of 32, else BH_ERR_INVALID_ARG).  The reference has no twin: it is k calls of multiexp,
 * which is also what every result and return code is defined by.  Proofs of one circuit share their bases and density
 * maps and differ in the scalars only; the many-plan pays the launch chain of a multiexp once - one digit stage, one sort,
 * one accumulate launch, one reduction, vector v taking the place of a window (table flavour: one bucket set per vector;
 * classic flavour: ceil(256 / c) sets per vector) - and runs the serial tail per vector on the host.
 *   dispatch   k = 0: BH_OK, nothing is written.  k = 1, and the host entry with n_scalars <= 8 (answered on the host at
 *              issue time), never use the many-plan.  Otherwise a size rule chooses between the many-plan and k ordinary
 *              jobs issued together and waited in order inside the same call; the rule is taken from
 *              profiles/msm_many_bench.json and is "never" where the many-plan was not measured faster: it takes the
 *              many-plan for 4 <= k <= 16 vectors of 2^10 ... 2^18 scalars over bases that have a window table.  A plan
 *              the rule chose and the pipeline or the pool cannot serve falls back to the ordinary jobs: the default
 *              call accepts every k that k calls of bh_msm_async_dev accept.
 *              BH_MSM_MANY_FORCE in opts.flags takes the many-plan wherever it is valid (k >= 2, n_scalars >= 1, and
 *              the 32-bit limits: bucket sets x entries per set < 2^32, at most 65535 sets, base index < 2^31 - beyond
 *              them BH_ERR_INVALID_ARG); BH_MSM_NO_TABLE forces its classic flavour.  BH_MSM_HOLD is BH_ERR_INVALID_ARG.
 *   limits     a many-plan job counts as ONE job under max_jobs_in_flight.
 *   after_stream (optional) as in bh_msm_async_dev_after.  The host entry uploads the k vectors and the density map once
 *              and keeps them until the wait; it returns when that upload has finished (unlike bh_msm_async, whose
 *              copy rides the job's stream) - the caller's arrays may be reused at once.  A many-plan job whose W * c
 *              result records do not fit the 256 KB pinned buffer of a job's resources replaces that buffer at issue
 *              time, which waits for the device once per growth; the larger buffer stays with the recycled resources.
 *   wait       k affine records and k return codes: BH_OK / BH_ERR_UNEXPECTED_IDENTITY / BH_ERR_UNEXPECTED_EOF, each
 *              exactly what the single call returns for that vector; a failed vector's record is all-zero.  The device
 *              status flags of a many-plan job are per JOB: if either is set once the job has run, every vector is
 *              answered again by the single-vector path over the still-resident inputs (errors are rare; this gives each
 *              vector the reference's precedence rule).  The return value carries call-level outcomes only (BH_OK,
 *              BH_ERR_INVALID_ARG, BH_ERR_HIP), as for bh_groth16_verify_each.  stage_ms4 and stats8 are optional and describe
 *              the whole job as bh_msm_wait_stats does (k ordinary jobs: the sums of [0..3], the plan of the last).
 *              scalars, density (device entry) and bases stay valid until the wait. */
typedef struct bh_msm_many_job bh_msm_many_job;
#define BH_MSM_MANY_FORCE 512u /* bh_msm_many_*: take the many-plan wherever it is valid */
int bh_msm_many_async_dev(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_dev, size_t stride_bytes,
                          size_t n_scalars, size_t k, int scalar_fmt, const uint64_t *density_words_dev, size_t density_len,
                          const bh_msm_opts *opts, void *after_stream, bh_msm_many_job **job);
int bh_msm_many_async(bh_ctx *ctx, const bh_bases *bases, size_t skip, const void *scalars_host, size_t stride_bytes,
                      size_t n_scalars, size_t k, int scalar_fmt, const uint64_t *density_words, size_t density_len,
                      const bh_msm_opts *opts, bh_msm_many_job **job);
int bh_msm_many_wait(bh_msm_many_job *job, void *out_affine_k, int32_t *rcs_k, float *stage_ms4, uint64_t *stats8);
/* The plan a many-job of k vectors of n scalars would run (host only, no context): table_bits = 0 the classic flavour,
 * else the table flavour over a window table of that many bits; num_cus = 0: 256.  out12 = c, bucket sets W, buckets per
 * set, K, chunks per set, sort passes, entries per set, vectors, sets per vector, digit columns per scalar, and the bytes
 * of the job's result buffer (low, high word).  BH_ERR_INVALID_ARG beyond the 32-bit limits above. */
int bh_msm_many_plan_info(size_t n, size_t k, int group, unsigned table_bits, unsigned num_cus, unsigned *out12);

/* ---- scalar vectors resident in HBM ------------------------------------------------------------------
 * create_proof hands the same `Arc<Vec<Exponent>>` to several multiexps (groth16/src/prover.rs:267,279,285,300,306,
 * 316,318: input_assignment to three, aux_assignment to four): registered once, uploaded once.  scalar_fmt as for
 * bh_msm_async - with BH_SCALARS_MONT a Rust `Vec<Scalar>` is handed over as is and the serial Fr -> Exponent pass of
 * prover.rs:241-261 disappears (the conversion happens on the device inside the digit kernel). */
typedef struct bh_scalars bh_scalars;
int bh_scalars_register(bh_ctx *ctx, const void *scalars_host, size_t n, int scalar_fmt, bh_scalars **out);
/* the same over an existing device vector; take_ownership != 0: the vector came from bh_dev_alloc of this context and
 * is returned to it by bh_scalars_release */
int bh_scalars_adopt_dev(bh_ctx *ctx, void *scalars_dev, size_t n, int scalar_fmt, int take_ownership, bh_scalars **out);
/* release after every multiexp issued over the handle has been waited on */
void bh_scalars_release(bh_scalars *s);
size_t bh_scalars_len(const bh_scalars *s);
const void *bh_scalars_dev_ptr(const bh_scalars *s);
/* multiexp over scalars [first, first + n) of a registered vector; the density map (NULL = FullDensity) is given on
 * the HOST as for bh_msm_async and describes exactly those n scalars; opts may be NULL */
int bh_msm_async_scalars(bh_ctx *ctx, const bh_bases *bases, size_t skip, const bh_scalars *scalars, size_t first,
                         size_t n, const uint64_t *density_words, size_t density_len, const bh_msm_opts *opts,
                         bh_msm_job **job);
/* The h block of create_proof (groth16/src/prover.rs:221-245) with the result LEFT IN HBM: a, b, c = n_evals
 * constraint evaluations (Montgomery Fr, host); *h_out = the m - 1 quotient coefficients (Montgomery) as a registered
 * scalar vector, ready for the H multiexp - no download, no Fr -> Exponent pass (prover.rs:241-242), no re-upload. */
int bh_h_poly_fr_scalars(bh_ctx *ctx, const void *a_host, const void *b_host, const void *c_host, size_t n_evals,
                         bh_scalars **h_out);

/* ---- one multiexp over several GPUs of ONE process (the reference is a single process,
 * src/multicore.rs:21-92) ------------------------------------------------------------------------
 * ctxs[k] = a context on GPU k (bh_ctx_create(k)), shards[k] = the k-th contiguous piece of the base vector,
 * registered on ctxs[k]; the concatenation of the shards is the `bases` of multiexp(pool, (bases, skip), density,
 * exponents).  The call cuts the exponents where the base index skip + rank_i crosses a shard boundary (re-basing the
 * density map), issues one job per shard - each GPU runs the whole single-GPU pipeline on its piece, there is no
 * device-to-device exchange - and bh_msm_sharded_wait folds the per-shard results (96 / 192 bytes each) on the
 * host.  Result and error semantics are those of ONE multiexp over the whole vector, including "EOF vs. identity:
 * the top window's first failure wins" (src/multiexp.rs:295-300) with the window size of the whole length.  Several
 * contexts on the same device are allowed (tests on a single-GPU box). */
typedef struct bh_msm_sharded_job bh_msm_sharded_job;
int bh_msm_sharded_async(bh_ctx *const *ctxs, const bh_bases *const *shards, size_t n_shards, size_t skip,
                         const void *scalars_host, size_t n_scalars, int scalar_fmt, const uint64_t *density_words,
                         size_t density_len, bh_msm_sharded_job **job);
int bh_msm_sharded_wait(bh_msm_sharded_job *job, void *out_affine);

/* ---- fixed-base scalar multiplication (fixture / CRS generation; SURVEY §8 f4,
 * groth16/src/generator.rs:271-296,398-421): out[i] = [s_i] base, affine records on device.  Windowed like the
 * reference's (a table of d * 2^(8j) * base is built on the device in front of the multiplications: at most 32 mixed
 * additions per scalar, no doublings); the call returns when the results are in out_dev (it waits for the stream). */
int bh_fixed_base_mul_dev(bh_ctx *ctx, int group, const void *base_affine_host,
                          const void *scalars_dev, size_t n, int scalar_fmt, void *out_dev,
                          void *stream);
/* ---- variable-base scalar multiplication, one scalar per point: out[i] = [s_i] in[i] over affine records on the device
 * (identity = the all-zero record; the points are NOT validated and must lie in the prime-order subgroup, where the
 * endomorphism acts as a scalar).  The split-scalar ladder of csrc/glv.cuh: s = s1 + s2 lambda with two 128-bit halves,
 * 128 joint double-and-add steps over a free three-entry table (csrc/point_mul.hip) instead of the 255
 * steps of bh_point_mul_assign_dev.  scalars_dev: n scalars of 32 bytes in scalar_fmt (a canonical-format value is taken
 * mod q).  out_dev may be in_dev.  The call returns when the results are in out_dev (it waits for the stream); n = 0 does
 * nothing; a bad group or format is BH_ERR_INVALID_ARG. */
int bh_point_mul_each_dev(bh_ctx *ctx, int group, const void *in_dev, const void *scalars_dev, size_t n, int scalar_fmt,
                          void *out_dev, void *stream);

/* ---- groth16::create_proof (groth16/src/prover.rs:182-361) --------------------------------------
 * bh_params = `&Parameters` as ParameterSource (groth16/src/lib.rs:435-473): the verifying-key
 * elements the prover uses plus the five query vectors (h, l, a, b_g1, b_g2), registered in HBM.
 * A proof is written as affine records a (96 B) | b (192 B) | c (96 B).
 * The C++ mirror of Circuit / ConstraintSystem / LinearCombination / ProvingAssignment lives in
 * bellman_amd/csrc/groth16.hpp; these entry points expose it to other host languages. */
typedef struct bh_params bh_params;
typedef struct bh_r1cs bh_r1cs; /* constraint matrices on the device, see the R1CS section below */
int bh_groth16_params_create(bh_ctx *ctx, const void *alpha_g1, const void *beta_g1, const void *beta_g2,
                             const void *delta_g1, const void *delta_g2, const void *h, size_t nh,
                             const void *l, size_t nl, const void *a, size_t na, const void *b_g1,
                             size_t nb1, const void *b_g2, size_t nb2, bh_params **out);
/* Parameters::read(reader, checked) (groth16/src/lib.rs:289-398, with VerifyingKey::read :159-215) on
 * the serialized CRS (`Parameters::write`, :258-287): decoding, and with checked != 0 the on-curve /
 * subgroup validation of the query points, run on the device; the verifying key is always validated.
 * The first failure in stream order is returned, as the reference's sequential reader would:
 * BH_ERR_INVALID_POINT, BH_ERR_POINT_AT_INFINITY (query and ic points must not be the identity) or
 * BH_ERR_UNEXPECTED_EOF (input ends inside the structure). Trailing bytes are ignored. */
int bh_groth16_params_read(bh_ctx *ctx, const void *bytes, size_t len, int checked, bh_params **out);
/* generate_parameters (groth16/src/generator.rs:163-510) for the circuit whose matrices are `r1cs`
 * (bh_r1cs_create; the matrices include the `input_i * 0 = 0` rows, generator.rs:195-202): g1 / g2 =
 * affine generators (96 / 192 B), alpha..tau = Montgomery Fr.  Everything per-variable or
 * per-constraint runs on the device.  BH_ERR_UNEXPECTED_IDENTITY for gamma = 0 or delta = 0 (:227-243),
 * BH_ERR_UNCONSTRAINED_VARIABLE (:464-470), BH_ERR_DEGREE_TOO_LARGE. */
int bh_groth16_generate(bh_ctx *ctx, bh_r1cs *r1cs, const void *g1, const void *g2, const void *alpha,
                        const void *beta, const void *gamma, const void *delta, const void *tau,
                        bh_params **out);
/* Parameters::write (groth16/src/lib.rs:258-287).  buf == NULL: *len = bytes needed.  Parameters made by
 * bh_groth16_params_create carry no gamma_g2 / ic and write them as the identity / an empty list. */
int bh_groth16_params_write(const bh_params *p, void *buf, size_t cap, size_t *len);
/* verifier-side key elements kept by params_read / generate: gamma_g2 (192 B), ic (n_ic x 96 B) */
int bh_groth16_params_vk_ext(const bh_params *p, void *gamma_g2, void *ic_out, size_t ic_cap, size_t *n_ic);
/* which: 0 h, 1 l, 2 a, 3 b_g1, 4 b_g2 - the device-resident query (owned by the params) and its length */
int bh_groth16_params_query(const bh_params *p, int which, const bh_bases **bases, size_t *len);
/* the prover-side verifying-key elements as affine Montgomery records (any pointer may be NULL) */
int bh_groth16_params_vk(const bh_params *p, void *alpha_g1, void *beta_g1, void *beta_g2, void *delta_g1,
                         void *delta_g2);
/* Proof::write (groth16/src/lib.rs:38-46): affine a | b | c (384 B) -> compressed A (48) | B (96) | C (48) */
void bh_proof_write(const void *proof_affine, void *out192);
void bh_groth16_params_release(bh_params *p);
/* prover.rs:217-360 on the fields of a synthesised ProvingAssignment (prover.rs:57-71): a/b/c
 * evaluations (n_constraints, input constraints of :208-215 already appended), input/aux
 * assignments (Montgomery Fr), the three density bitmaps (LSB0 words), r and s (Montgomery Fr).
 * timings4 (optional): [synthesis, h block, multiexps, total] host milliseconds. */
int bh_groth16_prove_assignment(bh_params *params, const void *a_evals, const void *b_evals,
                                const void *c_evals, size_t n_constraints, const void *input_assignment,
                                size_t n_inputs, const void *aux_assignment, size_t n_aux,
                                const uint64_t *a_aux_density, const uint64_t *b_input_density,
                                const uint64_t *b_aux_density, const void *r, const void *s,
                                void *proof_out, float *timings4);
/* ---- groth16 verification (groth16/src/verifier.rs, groth16/src/verifier/batch.rs) ---------------------------------
 * bh_pvk = PreparedVerifyingKey (groth16/src/lib.rs:400-409): the Miller-loop line coefficients of -gamma, -delta and beta
 * kept in HBM, and ic registered as multiexp bases.  Points are affine Montgomery records as everywhere in this header
 * (identity = all zero); a proof is affine a | b | c (384 B), the layout bh_groth16_prove_* write.
 *   bh_groth16_prepare_verifying_key  prepare_verifying_key (verifier.rs:11-21); n_ic >= 1.  BH_ERR_INVALID_POINT when
 *                                     beta / gamma / delta is not on the curve.
 *   bh_groth16_pvk_from_params        the same from the key elements of params made by bh_groth16_params_read or
 *                                     bh_groth16_generate (BH_ERR_INVALID_ARG for params without gamma_g2 / ic).
 *   bh_groth16_verify                 verify_proof (verifier.rs:23-58): BH_OK, BH_ERR_INVALID_PROOF, or first
 *                                     BH_ERR_INVALID_VERIFYING_KEY when n_inputs + 1 != the length of ic.
 *   bh_groth16_batch_verify           batch::Verifier::verify (batch.rs:93-192) over n_proofs proofs with n_inputs public
 *                                     inputs each (inputs row-major, n_proofs x n_inputs) and the caller's random
 *                                     z_j (n_proofs Fr from a CSPRNG, all nonzero: a z_j that is 0 mod q gives BH_ERR_INVALID_ARG).
 *                                     An empty batch is BH_OK.  Runs in chunks of at most 16384 proofs and 256 MB of inputs (bounded
 *                                     device workspace),
 *                                     on its own stream: thread-safe and concurrent with other work on the context.
 * scalar_fmt applies to inputs and z as for bh_msm_async.  The only point check these two AFFINE entry points make is the
 * on-curve test of A, B and C (BH_ERR_INVALID_POINT, reported before BH_ERR_INVALID_PROOF): for them subgroup membership,
 * which the reference's Proof::read guarantees through from_compressed, stays with the caller.  bh_proofs_read and
 * bh_groth16_batch_verify_compressed below take the proofs as Proof::write emits them and make every check of Proof::read. */
typedef struct bh_pvk bh_pvk;
int bh_groth16_prepare_verifying_key(bh_ctx *ctx, const void *alpha_g1, const void *beta_g2, const void *gamma_g2,
                                     const void *delta_g2, const void *ic, size_t n_ic, bh_pvk **out);
int bh_groth16_pvk_from_params(const bh_params *p, bh_pvk **out);
/* number of public inputs the key expects (ic length - 1) */
size_t bh_groth16_pvk_num_inputs(const bh_pvk *pvk);
int bh_groth16_verify(const bh_pvk *pvk, const void *proof, const void *inputs, size_t n_inputs, int scalar_fmt);
int bh_groth16_batch_verify(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                            int scalar_fmt, const void *z);
/* Proof::read (groth16/src/lib.rs:47-99) over n_proofs concatenated 192-byte proofs (compressed A 48 | B 96 | C 48, what
 * bh_proof_write emits), on the device: every point decompressed and checked (encoding, square root, prime-order subgroup),
 * the identity refused.  Writes n_proofs x 384 bytes of affine a | b | c, the layout bh_groth16_verify / _batch_verify take
 * (an element that fails is written as the all-zero record).  Returns BH_OK, or the error of the FIRST bad proof in stream
 * order and inside it of the first bad element in the order a, b, c - what the reference's sequential reader reports:
 * BH_ERR_INVALID_POINT ("invalid G1" / "invalid G2": bad encoding, no square root, outside the subgroup) or
 * BH_ERR_POINT_AT_INFINITY (a well-formed identity); *bad_index (optional) is that proof's position.
 * status (optional, one word per proof, written for EVERY proof whatever the return code; 0 = good proof) holds one byte
 * per element - bits 0-7 a, 8-15 b, 16-23 c - of these bits (csrc/msm_types.hpp PointStatus):
 *   0x02 sort flag on an infinity encoding   0x04 a coordinate >= p   0x08 infinity flag with coordinate bits set
 *   0x10 a well-formed identity ("point at infinity"; every other bit means "invalid")
 *   0x20 x^3 + b is not a square   0x40 not in the prime-order subgroup   0x80 compression flag clear
 * Runs in chunks of at most 16384 proofs on a stream of its own: thread-safe.  n_proofs = 0 is BH_OK. */
#define BH_PROOF_STATUS_IDENTITY 0x10u
#define BH_PROOF_STATUS_INVALID 0xeeu
int bh_proofs_read(bh_ctx *ctx, const void *bytes, size_t n_proofs, void *out_proofs_affine, uint32_t *status,
                   size_t *bad_index);
/* Proof::read of every proof followed by batch::Verifier::verify, without the decoded proofs visiting the host: 192 bytes
 * per proof are uploaded and decoded on the verifier's stream into the records the chunk pipeline of
 * bh_groth16_batch_verify consumes (same chunks, same bounded workspace, thread-safe and concurrent with other work on the
 * context like it).  Errors in this order: the argument errors of bh_groth16_batch_verify (input count, a z_j = 0 mod q),
 * then read errors as bh_proofs_read reports them (with *bad_index, optional) - a read error ANYWHERE in the batch wins
 * over BH_ERR_INVALID_PROOF, as for a caller of the reference who reads all proofs before queueing them - then the
 * verdict.  The batch is walked once: each chunk is decoded right before its Miller loops, and the first chunk that
 * holds a bad proof ends the call (the verdict exists only after the last chunk). */
int bh_groth16_batch_verify_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                       size_t n_inputs, int scalar_fmt, const void *z, size_t *bad_index);
/* Per-proof verdicts for n_proofs proofs of one key in one call: batch::Item::verify_single (groth16/src/verifier/batch.rs:55-66,
 * "for fallback logic when batch verification fails"), which is verify_proof (groth16/src/verifier.rs:23-58), for every proof.
 * proofs: n_proofs x 384 B affine a | b | c; inputs: row-major n_proofs x n_inputs (row j belongs to proof j), scalar_fmt as
 * for bh_groth16_verify.  verdicts[j] is exactly the code bh_groth16_verify(pvk, proof_j, inputs_j, n_inputs, scalar_fmt)
 * returns for that proof alone: BH_OK, BH_ERR_INVALID_POINT (A, B or C off its curve; before BH_ERR_INVALID_PROOF) or
 * BH_ERR_INVALID_PROOF; an all-zero identity record counts as it does there.  A bad proof never ends the walk.
 * The return value carries call-level outcomes only: BH_ERR_INVALID_VERIFYING_KEY first when n_inputs + 1 != the length of
 * ic, BH_ERR_INVALID_ARG, BH_ERR_HIP, and BH_OK whenever every verdict was written - even if every proof is bad.
 * *n_bad (optional) = the number of nonzero verdicts; n_proofs = 0 is BH_OK with *n_bad = 0.
 * Every proof takes one lane on the device (fixed-base accumulation of its inputs over a window table of ic kept with the
 * key, three Miller loops under shared squarings, its own final exponentiation): no host loop over proofs.  Runs in chunks
 * of at most 16384 proofs (bounded workspace) on a stream of its own: thread-safe and concurrent with other work on the
 * context, like the batch verifier.  The key's table is built by the first call (once, under std::call_once) and counts
 * against the context's table budget (bh_ctx_set_limits); a table that would not fit is built with a narrower window. */
int bh_groth16_verify_each(const bh_pvk *pvk, const void *proofs, size_t n_proofs, const void *inputs, size_t n_inputs,
                           int scalar_fmt, int32_t *verdicts, size_t *n_bad);
/* The same over n_proofs x 192 B as Proof::write emits them; the decoded proofs never visit the host.  verdicts[j] is what
 * bh_proofs_read returns for those 192 bytes alone if it fails (BH_ERR_INVALID_POINT / BH_ERR_POINT_AT_INFINITY), otherwise
 * what bh_groth16_verify returns on the decoded proof (batch.rs:55-66, verifier.rs:23-58 after groth16/src/lib.rs:47-99).
 * status[j] (optional) is the word bh_proofs_read writes for proof j.  The proofs after a bad one are still judged. */
int bh_groth16_verify_each_compressed(const bh_pvk *pvk, const void *bytes, size_t n_proofs, const void *inputs,
                                      size_t n_inputs, int scalar_fmt, int32_t *verdicts, uint32_t *status, size_t *n_bad);
/* before bh_ctx_destroy of the key's context (the key's device memory lives in the context's pool) */
void bh_groth16_pvk_release(bh_pvk *pvk);
/* ---- proofs of several verifying keys in one call -------------------------------------------------------------------
 * bh_pvk_set: 1 .. BH_PVK_SET_MAX_KEYS prepared keys of ONE context, addressed by their position.  The caller keeps
 * owning the keys; they must outlive the set.  The same key may appear twice.  bh_groth16_pvk_set_create returns
 * BH_ERR_INVALID_ARG for a null entry, keys of different contexts, or n_keys outside 1 .. BH_PVK_SET_MAX_KEYS.  The set
 * owns one small device table of per-key descriptors (the key's lines and flags, alpha, input count; and, once a
 * bh_groth16_verify_each_keys* call has needed them, the key's ic window table, its width, ic_0 and f(-alpha, beta)).  What
 * bh_groth16_verify_each adds to a key is still built once per KEY, by the first call that needs it, single-key or
 * multi-key; the table budget and the 8 / 4 / 2 / 1-bit fallback apply per key, so keys of one set may have different
 * widths.  A set is immutable once its descriptors are written: usable from several threads at once.  Release the set
 * before its keys and before bh_ctx_destroy.
 *
 * In the calls below proof j belongs to key key_of[j] (a position in the set).  `inputs` is RAGGED: the concatenation, in
 * proof order, of bh_groth16_pvk_num_inputs(key key_of[j]) scalars for proof j; n_inputs_total must equal that sum.
 * Call-level errors, before any work and before any output is written: BH_ERR_INVALID_ARG (a null set or key_of, a scalar
 * format, some key_of[j] >= bh_groth16_pvk_set_len), then BH_ERR_INVALID_VERIFYING_KEY when n_inputs_total is not the sum
 * (batch.rs:101-107 for every proof's own key), then BH_ERR_INVALID_ARG for any other null argument that is needed.
 * n_proofs = 0 is BH_OK.  Rows are grouped by key on the host for the
 * device (every 64-lane block works for one key) and results return in the caller's order: the outcome does not depend
 * on how the keys interleave. */
#define BH_PVK_SET_MAX_KEYS 64
typedef struct bh_pvk_set bh_pvk_set;
int bh_groth16_pvk_set_create(const bh_pvk *const *pvks, size_t n_keys, bh_pvk_set **out);
/* the number of keys (0 for NULL) */
size_t bh_groth16_pvk_set_len(const bh_pvk_set *set);
void bh_groth16_pvk_set_release(bh_pvk_set *set);
/* verdicts[j] is the code bh_groth16_verify(key key_of[j], proof_j, inputs_j, its input count, scalar_fmt) returns for that
 * proof alone.  Return value, *n_bad and chunking as for bh_groth16_verify_each: chunks of at most 16384 proofs, each on the
 * call's own stream with one download and one synchronisation; thread-safe. */
int bh_groth16_verify_each_keys(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, size_t n_proofs,
                                const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts, size_t *n_bad);
/* The same over n_proofs x 192 B as Proof::write emits them: verdicts[j] and status[j] (optional) are what
 * bh_groth16_verify_each_compressed defines for proof j under key key_of[j]. */
int bh_groth16_verify_each_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                           const void *inputs, size_t n_inputs_total, int scalar_fmt, int32_t *verdicts,
                                           uint32_t *status, size_t *n_bad);
/* The batch check over proofs of several keys.  With E_j the value whose being 1 is proof j's verification equation under
 * its own key, BH_OK exactly when prod_j E_j^{z_j} = 1: the product over the keys of the values bh_groth16_batch_verify
 * tests key by key, under ONE final exponentiation.  Everything else as in the single-key call: a z_j that is 0 mod q gives
 * BH_ERR_INVALID_ARG, a point off its curve BH_ERR_INVALID_POINT (before BH_ERR_INVALID_PROOF).  A key of the set that has
 * no proof in the batch takes no part.
 * THE z_j MUST BE DRAWN AFTER THE BATCH IS FIXED, from a CSPRNG, and the rule holds ACROSS keys: whoever knows z beforehand
 * can make the errors of bad proofs cancel - inside one key, as in bh_groth16_batch_verify, and equally between proofs of
 * DIFFERENT keys, since all of them meet in one product. */
int bh_groth16_batch_verify_keys(const bh_pvk_set *set, const uint32_t *key_of, const void *proofs, size_t n_proofs,
                                 const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z);
/* The same from the bytes of Proof::write, as bh_groth16_batch_verify_compressed: a proof that fails to read ends the call
 * with the reader's code for the first such proof of its chunk in the CALLER's order, and *bad_index (optional) is its
 * position in the caller's order. */
int bh_groth16_batch_verify_keys_compressed(const bh_pvk_set *set, const uint32_t *key_of, const void *bytes, size_t n_proofs,
                                            const void *inputs, size_t n_inputs_total, int scalar_fmt, const void *z,
                                            size_t *bad_index);
/* ---- R1CS resident in HBM: constraint evaluation as sparse matrix x witness --------
 * The reference evaluates the A/B/C linear combinations of every constraint on one host thread
 * during synthesis (groth16/src/prover.rs:19-55 `eval`, :105-145 `enforce`).  The matrices are a
 * property of the circuit (like the CRS), so they are registered once; per proof only the witness
 * is uploaded and a = A.w, b = B.w, c = C.w are computed on the device, where the h block consumes
 * them.  Row i of a matrix holds terms [row_ptr[i], row_ptr[i+1]); a term is (var, coeff): var <
 * n_inputs addresses input_assignment[var], otherwise aux_assignment[var - n_inputs]; coeff indexes
 * `coeffs` (n_coeffs Montgomery Fr, coeffs[0] must be 1).  Terms with a zero coefficient contribute
 * neither to the value nor to the query densities (prover.rs:31).  n_constraints includes the
 * `input_i * 0 = 0` rows that create_proof appends (prover.rs:208-215). */
typedef struct {
  const uint32_t *row_ptr; /* n_constraints + 1 */
  const uint32_t *var;     /* nnz */
  const uint32_t *coeff;   /* nnz */
} bh_csr;
int bh_r1cs_create(bh_ctx *ctx, size_t n_inputs, size_t n_aux, size_t n_constraints, const bh_csr abc[3],
                   const void *coeffs, size_t n_coeffs, bh_r1cs **out);
void bh_r1cs_release(bh_r1cs *r);
int bh_r1cs_shape(const bh_r1cs *r, size_t *n_inputs, size_t *n_aux, size_t *n_constraints);
/* which: 0 a_aux_density, 1 b_input_density, 2 b_aux_density (prover.rs:59-61): LSB0 words on the
 * device / on the host, and get_total_density() (multiexp.rs:154-156).  Any out pointer may be NULL. */
int bh_r1cs_density(const bh_r1cs *r, int which, const uint64_t **dev_words, const uint64_t **host_words,
                    size_t *total);
/* a/b/c[0 .. 2^log_m) <- constraint evaluations (Montgomery), zero above n_constraints
 * (EvaluationDomain::from_coeffs padding, domain.rs:68).  Asynchronous on `stream`. */
int bh_r1cs_eval_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, const void *aux_dev,
                     void *a_dev, void *b_dev, void *c_dev, uint32_t log_m, void *stream);
/* ---- k witnesses of one circuit in one call: the evaluation above, and the CHECK that a witness satisfies the circuit -----
 * (the reference: TestConstraintSystem::which_is_unsatisfied / is_satisfied, src/gadgets/test/mod.rs:254-272 - the first
 * constraint in order with a * b != c; the provers above accept any witness of the right length and divide a * b - c by Z
 * without asking whether it divides).  Witness j is inputs_dev + j * in_stride and aux_dev + j * aux_stride: strides in
 * BYTES, multiples of 32 and at least the vector's length - the layout of bh_msm_many_async_dev and
 * bh_h_poly_fr_many_dev_on.  A lane reads every term record and coefficient once per tile of witnesses, not once per
 * witness.  BH_ERR_INVALID_ARG for a null handle or buffer, a stride below the vector's length or not a multiple of 32, and
 * 2^log_m < n_constraints; k = 0 is BH_OK and launches nothing.
 *   bh_r1cs_eval_many_dev   a/b/c_dev + j * out_stride (out_stride >= 2^log_m * 32) receive exactly what bh_r1cs_eval_dev
 *                           writes for witness j, zero padding up to 2^log_m included; nothing beyond 2^log_m records of a
 *                           vector is written.  Asynchronous on `stream`.
 *   bh_r1cs_check_many_dev  first_bad_dev[j] = the index of the first constraint witness j does not satisfy, or
 *                           BH_R1CS_SATISFIED.  No a, b or c vector is written: the call needs no workspace.  Asynchronous
 *                           on `stream`.
 *   bh_r1cs_check_many      the same from the host: witness j at inputs_host + j * n_inputs * 32 and aux_host + j * n_aux *
 *                           32, uploaded in groups that stay within 1 GiB of device memory.  Synchronous, on a stream of its
 *                           own: thread-safe.
 * When to call it: before bh_groth16_prove_witness* whenever the witness comes from code that is not yet trusted - a wrong
 * wire otherwise yields a well-formed proof that fails verification, and nothing names the constraint. */
#define BH_R1CS_SATISFIED 0xFFFFFFFFu /* n_constraints < 2^32, so never an index */
int bh_r1cs_eval_many_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, size_t in_stride, const void *aux_dev,
                          size_t aux_stride, size_t k, void *a_dev, void *b_dev, void *c_dev, size_t out_stride,
                          uint32_t log_m, void *stream);
int bh_r1cs_check_many_dev(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_dev, size_t in_stride, const void *aux_dev,
                           size_t aux_stride, size_t k, uint32_t *first_bad_dev, void *stream);
int bh_r1cs_check_many(bh_ctx *ctx, const bh_r1cs *r, const void *inputs_host, const void *aux_host, size_t k,
                       uint32_t *first_bad_host);
/* ---- the witness itself: k witnesses completed on the device from the values the caller supplies ------------------------
 * (the reference computes every variable in a closure on one host thread, groth16/src/prover.rs:57-103).  `alloc` followed
 * by `enforce(a, b, c)` with the new variable alone in c - AllocatedNum::mul, AllocatedBit::and / xor, packing, a MiMC round -
 * determines that variable from the matrices: v = (<A_i, w> <B_i, w> - rest of C_i) / s_v.  A solver is derived once per
 * circuit from a bh_r1cs, which must outlive it.  Variable indices are those of bh_csr.var (0 is ONE).
 *   known from the start   ONE, the `supplied` variables, every output variable of a hint
 *   one sweep, in order    constraint i defines v when v is the only variable of A_i, B_i, C_i not yet known (terms with a
 *                          zero coefficient do not count), v has no term in A_i or B_i and the sum s_v of its coefficients in
 *                          C_i is not zero.  There is no second sweep: synthesis order needs none.
 *   hints                  values no constraint determines, from a linear combination lc_var / lc_coeff[lc_begin .. lc_end) over
 *                          a coefficient table of their own (hint_coeffs: Montgomery Fr, entry 0 must be 1):
 *                          BH_HINT_BITS         out_var[out_begin + j] = bit shift + j of the CANONICAL integer of the
 *                                               combination, as Fr 0 or 1; shift + count <= 256
 *                          BH_HINT_INV_OR_ZERO  the one output = the combination's inverse, or 0 when it is 0
 * bh_r1cs_solver_create returns BH_ERR_INVALID_ARG, and in *first_unsolved (may be NULL) the variable concerned or
 * 0xFFFFFFFF, when a variable stays unknown after the sweep (the lowest one: supply it or add a hint), when a hint writes
 * ONE, a supplied variable or another hint's output (that variable), when hints and constraints depend on one another in a
 * cycle (the lowest variable on or behind it), or when a hint record is malformed.
 * bh_r1cs_solver_info: counts = supplied variables, constraint-defined variables, hint outputs, dependency levels, the
 * definitions of the widest level.
 * bh_r1cs_solve_many_dev completes witness j at inputs_dev + j * in_stride, aux_dev + j * aux_stride (the layout and the
 * argument checks of bh_r1cs_check_many_dev) in place: it writes every defined and hinted variable whatever the buffer
 * held, and never ONE, a supplied variable or a byte between the vector's end and the stride.  It checks no constraint -
 * bh_r1cs_check_many_dev on the same buffers does.  Asynchronous on `stream`; k = 0 is BH_OK and launches nothing.
 * bh_r1cs_solve_many: the same from and to the host, witness j at j * n_inputs * 32 and j * n_aux * 32, in groups that stay
 * within 1 GiB of device memory.  Synchronous, on a stream of its own: thread-safe. */
#define BH_HINT_BITS 1u
#define BH_HINT_INV_OR_ZERO 2u
typedef struct bh_r1cs_solver bh_r1cs_solver;
typedef struct {
  uint32_t kind;      /* BH_HINT_* */
  uint32_t lc_begin;  /* the combination: terms [lc_begin, lc_end) of lc_var / lc_coeff */
  uint32_t lc_end;
  uint32_t out_begin; /* the outputs: out_var[out_begin .. out_end) */
  uint32_t out_end;
  uint32_t shift;     /* BH_HINT_BITS: the first bit; otherwise 0 */
} bh_witness_hint;
typedef struct {
  const uint32_t *supplied;
  size_t n_supplied;
  const bh_witness_hint *hints;
  size_t n_hints;
  const uint32_t *lc_var;
  const uint32_t *lc_coeff;
  const uint32_t *out_var;
  const void *hint_coeffs;
  size_t n_hint_coeffs;
} bh_solver_desc;
int bh_r1cs_solver_create(bh_ctx *ctx, const bh_r1cs *r, const bh_solver_desc *desc, uint32_t *first_unsolved,
                          bh_r1cs_solver **out);
void bh_r1cs_solver_release(bh_r1cs_solver *s);
int bh_r1cs_solver_info(const bh_r1cs_solver *s, size_t counts[5]);
int bh_r1cs_solve_many_dev(bh_ctx *ctx, const bh_r1cs_solver *s, void *inputs_dev, size_t in_stride, void *aux_dev,
                           size_t aux_stride, size_t k, void *stream);
int bh_r1cs_solve_many(bh_ctx *ctx, const bh_r1cs_solver *s, void *inputs_host, void *aux_host, size_t k);
/* ---- the witness of a gadget circuit from its WORD PROGRAM: k witnesses computed on the device from their external words --
 * (replaces the values `circuit.synthesize` computes in its closures, groth16/src/prover.rs:206, for circuits built from the
 * UInt32 gadgets of src/gadgets/uint32.rs: a SHA-256 block is ~26 000 one-bit variables that a few thousand 32-bit operations
 * determine).  A trace word is a u64; words 0 .. n_ext - 1 are EXTERNAL - one uint32 each per witness, e.g. the message -
 * and instruction j writes word n_ext + j from words below its own.  The 32-bit operations read the low 32 bits of their
 * sources and write a 32-bit value:
 *   BH_WORD_CONST  a = the value          BH_WORD_ROTR, BH_WORD_SHR  word a by b, 1 <= b <= 31      BH_WORD_XOR, BH_WORD_AND  words a, b
 *   BH_WORD_CH     (a & b) ^ (~a & c)     BH_WORD_MAJ  (a & b) ^ (a & c) ^ (b & c), words a, b, c
 *   BH_WORD_ADD    the FULL sum, up to 36 bits, of the low halves of words pool[a .. a + b), 2 <= b <= 10
 *   BH_WORD_PACK   bit i of the result = bit source bits[a + i], i < 32
 * A bit source is bit `bit_neg & 0xff` (below 64) of `word`, negated when bit 8 of bit_neg is set.  Every variable but ONE
 * (indices as bh_csr.var) has exactly one record: a bit variable (the field element 0 or 1 of its source) or a packed
 * variable (the sum of bit source bits[bits_begin + i] * 2^i over i < n_bits <= 254).
 * bh_word_witness_create validates the program (host code, csrc/word_program.hpp) and copies it to the device.  A refused
 * program gives BH_ERR_INVALID_ARG with bad_index[0] = the reason and bad_index[1] = what that reason counts (bad_index may
 * be NULL):
 *   BH_WORD_BAD_SOURCE        instruction: a source is not strictly earlier than its destination
 *   BH_WORD_BAD_BIT           instruction, a PACK: a bit index of 64 or more
 *   BH_WORD_BAD_ADD_ARITY     instruction, an ADD: fewer than 2 or more than 10 sources
 *   BH_WORD_BAD_OP            instruction: unknown operation, amount outside 1 .. 31, a range that leaves its pool
 *   BH_WORD_BAD_VAR_SOURCE    variable: its record names a word or a bit that does not exist
 *   BH_WORD_BAD_PACKED_BITS   variable: packed from more than 254 bits
 *   BH_WORD_BAD_VAR_RANGE     record, bit records counted first and packed records behind them: variable index out of range
 *   BH_WORD_BAD_UNCOVERED     variable: no record - the lowest such variable
 *   BH_WORD_BAD_COVERED_TWICE variable: two records, or a record for ONE
 * bh_word_witness_generate_dev writes witness j to inputs_dev + j * in_stride and aux_dev + j * aux_stride (the layout and
 * stride rules of bh_r1cs_solve_many_dev) from the n_ext uint32 at ext_dev + j * ext_stride (bytes, a multiple of 4): every
 * variable, ONE included, whatever the buffers held, and no byte between a vector's end and its stride.  The buffers are
 * what bh_r1cs_check_many_dev and bh_groth16_prove_witness_batch_dev read.  Asynchronous on `stream`; k = 0 is BH_OK.  A
 * handle owns the scratch its calls share (witnesses go through in chunks of bounded scratch): calls on one handle are
 * ordered one behind the other, on whatever streams they run.
 * bh_word_witness_generate: the same from and to the host, witness j at j * n_ext * 4, j * n_inputs * 32 and j * n_aux * 32,
 * in groups that stay within 1 GiB of device memory.  Synchronous, on a stream of its own. */
#define BH_WORD_CONST 1u
#define BH_WORD_ROTR 2u
#define BH_WORD_SHR 3u
#define BH_WORD_XOR 4u
#define BH_WORD_AND 5u
#define BH_WORD_CH 6u
#define BH_WORD_MAJ 7u
#define BH_WORD_ADD 8u
#define BH_WORD_PACK 9u
#define BH_WORD_BAD_SOURCE 1u
#define BH_WORD_BAD_BIT 2u
#define BH_WORD_BAD_ADD_ARITY 3u
#define BH_WORD_BAD_OP 4u
#define BH_WORD_BAD_VAR_SOURCE 5u
#define BH_WORD_BAD_PACKED_BITS 6u
#define BH_WORD_BAD_VAR_RANGE 7u
#define BH_WORD_BAD_UNCOVERED 8u
#define BH_WORD_BAD_COVERED_TWICE 9u
typedef struct bh_word_witness bh_word_witness;
typedef struct {
  uint32_t op; /* BH_WORD_* */
  uint32_t a;
  uint32_t b;
  uint32_t c;
} bh_word_instr;
typedef struct {
  uint32_t word;
  uint32_t bit_neg; /* bit | neg << 8 */
} bh_word_bit;
typedef struct {
  uint32_t var;
  uint32_t word;
  uint32_t bit_neg;
} bh_word_var;
typedef struct {
  uint32_t var;
  uint32_t bits_begin;
  uint32_t n_bits;
} bh_word_packed;
typedef struct {
  size_t n_inputs; /* ONE included */
  size_t n_aux;
  size_t n_ext;
  const bh_word_instr *instrs;
  size_t n_instrs;
  const uint32_t *pool;
  size_t n_pool;
  const bh_word_bit *bits;
  size_t n_bits;
  const bh_word_var *vars;
  size_t n_vars;
  const bh_word_packed *packed;
  size_t n_packed;
} bh_word_witness_desc;
int bh_word_witness_create(bh_ctx *ctx, const bh_word_witness_desc *desc, bh_word_witness **out, uint32_t bad_index[2]);
int bh_word_witness_generate_dev(bh_ctx *ctx, const bh_word_witness *w, const void *ext_dev, size_t ext_stride, void *inputs_dev,
                                 size_t in_stride, void *aux_dev, size_t aux_stride, size_t k, void *stream);
int bh_word_witness_generate(bh_ctx *ctx, const bh_word_witness *w, const void *ext_host, void *inputs_host, void *aux_host,
                             size_t k);
void bh_word_witness_destroy(bh_word_witness *w);
/* Parameter generation (groth16/src/generator.rs:247-462) - device building blocks:
 *   bh_fr_powers_dev             out[i] = scale * g^i           (:249-263 powers of tau; :266-296 with t(tau)/delta folded in)
 *   bh_r1cs_eval_transposed_dev  at/bt/ct[v] = QAP polynomial of variable v at tau (:369-387) from the
 *                                Lagrange coefficients (ifft of the powers of tau, :299-300); n_inputs + n_aux entries each
 *   bh_fr_qap_ext_dev            e[v] = (at*beta + bt*alpha + ct) * (v < n_inputs ? 1/gamma : 1/delta)   (:400-407)
 * followed by bh_fixed_base_mul_dev for the h, a, b_g1, b_g2, ic/l points.  Scalars are Montgomery Fr. */
int bh_fr_powers_dev(bh_ctx *ctx, void *out_dev, size_t n, const void *g_host, const void *scale_host, void *stream);
int bh_r1cs_eval_transposed_dev(bh_ctx *ctx, bh_r1cs *r, const void *lagrange_dev, void *at_dev, void *bt_dev,
                                void *ct_dev, void *stream);
int bh_fr_qap_ext_dev(bh_ctx *ctx, void *e_dev, const void *at_dev, const void *bt_dev, const void *ct_dev,
                      size_t n_inputs, size_t n_vars, const void *alpha, const void *beta, const void *gamma_inv,
                      const void *delta_inv, void *stream);
/* The QAP evaluation IN THE GROUP (csrc/r1cs_points.hip): out[v] = sum over the constraints j that use variable v in one
 * matrix (0 A, 1 B, 2 C) of coeff * L[j], for a device vector L of affine G1 / G2 records - the Lagrange-basis points
 * [L_j(tau)]G that bh_fft_point_dev(BH_IFFT) makes of a powers-of-tau transcript.  It is bh_r1cs_eval_transposed_dev
 * followed by bh_fixed_base_mul_dev for a caller who does not know tau.  lagrange_points_dev holds at least
 * n_constraints records, out_points_dev n_inputs + n_aux (identity = the all-zero record); accumulate != 0 adds the
 * product to what out_points_dev holds instead of overwriting it.  The points are NOT validated.  Enqueued on `stream`
 * (NULL = context stream); when the matrix has coefficients other than 0 and +-1 the call takes pool workspace for their
 * scalar multiples and waits for the stream before it returns. */
int bh_r1cs_eval_transposed_points_dev(bh_ctx *ctx, bh_r1cs *r, int group, int matrix, const void *lagrange_points_dev,
                                       void *out_points_dev, int accumulate, void *stream);
/* ---- parameters from a powers-of-tau transcript (what a deployment holds instead of tau, alpha, beta) ----------------
 * The transcript as device-resident handles: [tau^i]G1 (at least 2m - 1 points), [tau^i]G2, [alpha tau^i]G1 and
 * [beta tau^i]G1 (at least m each), m = the next power of two >= the circuit's constraint count (EvaluationDomain::
 * from_coeffs, src/domain.rs:47-79); longer vectors are fine, their prefix is used (one ceremony serves every smaller
 * circuit).  beta_g2 is one affine G2 record on the host. */
typedef struct {
  const bh_bases *tau_g1;
  const bh_bases *tau_g2;
  const bh_bases *alpha_tau_g1;
  const bh_bases *beta_tau_g1;
  const void *beta_g2;
} bh_powers_of_tau;
/* generate_parameters (groth16/src/generator.rs:163-510) in the exponent, with gamma = delta = 1: g1 = tau_g1[0],
 * g2 = tau_g2[0]; alpha_g1, beta_g1 = element 0 of their vectors; gamma_g2 = delta_g2 = g2, delta_g1 = g1;
 * h[i] = tau_g1[i + m] - tau_g1[i] (= [tau^i t(tau)]G1), i < m - 1; the four m-prefixes go through the point ifft, and
 * a, b_g1, b_g2, ic and l are the products of the circuit's transposed matrices with the resulting Lagrange points
 * (bh_r1cs_eval_transposed_points_dev).  The result is the same group elements, so the same Parameters::write bytes, as
 * bh_groth16_generate(alpha, beta, 1, 1, tau) for the scalars behind the transcript; bh_groth16_params_rescale_delta then
 * sets delta.  Identities are dropped from a, b_g1, b_g2 and an identity in l is BH_ERR_UNCONSTRAINED_VARIABLE, as there.
 * BH_ERR_INVALID_ARG for a null or wrong-group handle, BH_ERR_DEGREE_TOO_LARGE when a vector is too short.
 * THIS CALL VALIDATES NOTHING: neither that the points are on their curves and in the prime-order subgroups - read the
 * transcript with bh_bases_read_uncompressed / _compressed and BH_POINTS_CHECKED, or run bh_bases_validate over the
 * handles, for that - nor that the four vectors and beta_g2 are consistent powers of one (tau, alpha, beta), which takes
 * pairings: bh_powers_of_tau_verify below makes both checks.  Runs on a stream of its own: thread-safe and concurrent with other work on the context. */
int bh_groth16_generate_from_powers_of_tau(bh_ctx *ctx, bh_r1cs *r1cs, const bh_powers_of_tau *t, bh_params **out);
/* New parameters with delta multiplied by d (32-byte Montgomery Fr on the host): delta_g1 and delta_g2 are multiplied by d,
 * every point of h and l by 1/d (on the device; the new queries are registered like any other, so they get window
 * tables), a, b_g1, b_g2 and the rest of the key are copied.  `p` is left unchanged.  d = 0 -> BH_ERR_UNEXPECTED_IDENTITY.
 * Applied to the delta = 1 output of the call above it gives generate(alpha, beta, 1, d, tau); applied repeatedly it is
 * one contributor's step of a circuit-specific ceremony; the receiver checks the step with bh_groth16_params_verify_step
 * and the contribution proofs with bh_pairing_same_ratio_each (below). */
int bh_groth16_params_rescale_delta(const bh_params *p, const void *d_mont, bh_params **out);
/* ---- contributing to a transcript (what a phase-1 contributor runs; the receiver's side is bh_powers_of_tau_verify plus
 * bh_pairing_same_ratio_each below) --------------------------------------------------------------------------------------
 * bh_bases_scale_powers: a NEW handle with out[i] = [c g^i] in[i] for c, g Montgomery Fr on the host, by
 * bh_point_mul_each_dev's kernel over a device vector of the powers.  The handle is registered like any other (so it
 * gets the automatic window table) and is released with bh_bases_release; `in` is left unchanged.  c = 0 or g = 0 is
 * BH_ERR_UNEXPECTED_IDENTITY.  Runs on a stream of its own: thread-safe.
 * bh_powers_of_tau_contribute: out[0..3] = new handles T'[i] = [tau^i] T[i], U'[i] = [tau^i] U[i], A'[i] = [alpha tau^i]
 * A[i], B'[i] = [beta tau^i] B[i] over the WHOLE length of every vector of `before`, and beta_g2_out (192 bytes on the
 * host) = [beta] beta_g2 (bh_point_mul).  tau, alpha, beta: Montgomery Fr on the host, the contributor's secrets - the
 * caller erases them; a zero secret is BH_ERR_UNEXPECTED_IDENTITY, a null or wrong-group handle BH_ERR_INVALID_ARG; on
 * an error no handle is returned.  THIS CALL VALIDATES NOTHING: neither that the points are on their curves and in the
 * prime-order subgroups - read the transcript with bh_bases_read_uncompressed / _compressed and BH_POINTS_CHECKED, or run
 * bh_bases_validate over the handles, for that - nor that the four vectors and beta_g2 are consistent powers of one
 * (tau, alpha, beta), which takes pairings: bh_powers_of_tau_verify below makes both checks.  Each vector runs on a stream
 * of its own: thread-safe and concurrent with other work on the context. */
int bh_bases_scale_powers(bh_ctx *ctx, const bh_bases *in, const void *c_mont, const void *g_mont, bh_bases **out);
int bh_powers_of_tau_contribute(bh_ctx *ctx, const bh_powers_of_tau *before, const void *tau_mont, const void *alpha_mont,
                                const void *beta_mont, bh_bases *out[4], void *beta_g2_out);
/* ---- checking a transcript before deriving parameters from it -----------------------------------------------------------
 * bh_pairing_product_is_one: *is_one = (prod_i e(P_i, Q_i) == 1) over n pairs of affine records on the host (96 B / 192 B
 * each): the lines of every Q_i, one Miller lane per pair, the product, one final exponentiation - the verifier's kernels.
 * A pair with the identity on either side contributes 1; n = 0 gives 1.  A point off its curve is BH_ERR_INVALID_POINT, n
 * above 16384 BH_ERR_INVALID_ARG.  Subgroup membership stays with the caller, as for bh_groth16_verify.  Thread-safe (a
 * stream of its own).  The primitive of the transcript check below; a ceremony verifier checks contribution proofs with it. */
int bh_pairing_product_is_one(bh_ctx *ctx, const void *g1_affine_host, const void *g2_affine_host, size_t n, int *is_one);
/* bh_powers_of_tau_verify: are the four vectors and beta_g2 powers of ONE (tau, alpha, beta)?  With T = tau_g1 (at least 2
 * points), U = tau_g2 (at least 2), A = alpha_tau_g1, B = beta_tau_g1 (at least 1 each; a shorter vector is
 * BH_ERR_INVALID_ARG; the WHOLE length of every handle is checked), g1 = T[0], s1 = T[1], g2 = U[0], s2 = U[1], and for a
 * vector V of n points P(V) = sum_{i<n-1} rho_i V[i], Q(V) = sum_{i<n-1} rho_i V[i+1] (two multiexps over the same
 * coefficients, skip 0 and 1), the bits of report->failed are
 *   HEAD       one of g1, s1, g2, s2, A[0], B[0], beta_g2 is the identity or off its curve; nothing else is evaluated
 *   TAU_G1_G2  e(s1, g2) != e(g1, s2)                 TAU_G1   e(P(T), s2) != e(Q(T), g2)
 *   TAU_G2     e(s1, P(U)) != e(g1, Q(U))             ALPHA    e(P(A), s2) != e(Q(A), g2)   (vacuous for one point)
 *   BETA       the same for B                         BETA_G2  e(B[0], g2) != e(g1, beta_g2)
 *   POINTS     only with BH_PTAU_VALIDATE_POINTS in flags: the four vectors first go through bh_bases_validate with
 *              CHECKED | FORBID_IDENTITY; the first failure in the order T, U, A, B ends the call with bad_vector (0..3),
 *              bad_index and the return code BH_ERR_INVALID_POINT / BH_ERR_POINT_AT_INFINITY.
 * A multiexp that meets an identity (BH_ERR_UNEXPECTED_IDENTITY) sets its vector's bit: no consistent transcript holds
 * one.  Returns BH_OK when failed == 0, BH_ERR_INVALID_TRANSCRIPT when an equation bit (or HEAD) is set, otherwise the
 * usual call-level codes; without BH_PTAU_VALIDATE_POINTS a sum over records that are not on the curve can surface as
 * BH_ERR_INVALID_POINT.  report may be NULL.
 * The coefficients rho are expanded on the device from seed32 (csrc/ptau_rlc.cuh: BLAKE2s keyed with the seed, 128 bits
 * per coefficient).  THE SEED MUST BE CHOSEN AFTER THE TRANSCRIPT IS FIXED, AND FROM A CSPRNG: whoever knows it beforehand
 * can build an inconsistent transcript that passes - the counterpart of the z_j rule of bh_groth16_batch_verify.
 * The eight multiexps run together as ordinary jobs with the default plans (a window table is used where a handle has one;
 * none is built), all equations in one Miller launch.  Thread-safe and concurrent with other work on the context.
 * NOT COVERED by this call: a proof of knowledge of the contributors' secrets (contribution proofs:
 * bh_pairing_same_ratio_each), tau being a root of unity of the domain (such a transcript passes and gives unusable
 * parameters: compare tau_g1[m] with tau_g1[0] by bh_bases_first_difference), and the parsing of any ceremony's file format. */
#define BH_PTAU_VALIDATE_POINTS 1u
#define BH_PTAU_FAILED_HEAD 0x01u
#define BH_PTAU_FAILED_TAU_G1_G2 0x02u
#define BH_PTAU_FAILED_TAU_G1 0x04u
#define BH_PTAU_FAILED_TAU_G2 0x08u
#define BH_PTAU_FAILED_ALPHA 0x10u
#define BH_PTAU_FAILED_BETA 0x20u
#define BH_PTAU_FAILED_BETA_G2 0x40u
#define BH_PTAU_FAILED_POINTS 0x80u
typedef struct {
  uint32_t failed;
  uint32_t bad_vector;
  size_t bad_index;
} bh_ptau_report;
int bh_powers_of_tau_verify(bh_ctx *ctx, const bh_powers_of_tau *t, const void *seed32, unsigned flags, bh_ptau_report *report);
/* ---- checking a circuit-specific ceremony step (what the RECEIVER of bh_groth16_params_rescale_delta's output runs) ------
 * bh_bases_first_difference: *index = the first i < count at which record first_a + i of `a` differs from record
 * first_b + i of `b`, or `count` when the two ranges hold the same records.  Records are compared AS STORED (96 / 192
 * bytes, Montgomery, identity = the all-zero record): the resident form of every handle this library makes is the reduced
 * one (coordinates < p), so equal points are equal bytes; a record with a coordinate >= p differs from its reduced twin -
 * bh_bases_validate (status 0x04) is the call that finds such a record.  BH_OK whether or not a difference exists;
 * BH_ERR_INVALID_ARG for handles of different groups, a range beyond a handle, or a wrapped buffer that is not 16-byte
 * aligned; count = 0 gives *index = 0.  `a` and `b` may be the same handle.  One kernel launch of any length (one lane per
 * record, bandwidth-bound: csrc/bases_compare.cuh) on a stream of its own: thread-safe. */
int bh_bases_first_difference(bh_ctx *ctx, const bh_bases *a, size_t first_a, const bh_bases *b, size_t first_b, size_t count,
                              size_t *index);
/* bh_pairing_same_ratio_each: n independent equations over affine host records (96 B / 192 B each, row i of each array):
 * verdicts[i] = BH_OK iff e(a_i, B_i) == e(b_i, A_i), that is b_i / a_i = B_i / A_i - the "same ratio" test of a
 * contribution proof.  Otherwise BH_ERR_POINT_AT_INFINITY when any of the row's four points is the identity (a ratio
 * through the identity proves nothing - NOT the "contributes 1" rule of bh_pairing_product_is_one; tested first),
 * BH_ERR_INVALID_POINT when one of them is off its curve, BH_ERR_INVALID_TRANSCRIPT when the equation fails.  A bad row
 * never ends the walk and never changes another row's verdict.  The return value carries call-level outcomes only, as for
 * bh_groth16_verify_each: BH_OK whenever every verdict was written; *n_bad (optional) = the number of nonzero verdicts;
 * n = 0 is BH_OK.  Two Miller lanes per row, one fold launch, one final exponentiation per row in one launch; rows decided
 * on the host keep their lanes (with identity pairs).  Runs in chunks of at most 8192 rows on a stream of its own, for any
 * n: thread-safe.  Subgroup membership stays with the caller, as for bh_groth16_verify. */
int bh_pairing_same_ratio_each(bh_ctx *ctx, const void *a_g1, const void *b_g1, const void *A_g2, const void *B_g2, size_t n,
                               int32_t *verdicts, size_t *n_bad);
/* bh_groth16_params_verify_step: is `after` = `before` with delta multiplied by some unknown d != 0 and NOTHING else
 * changed - the check of one bh_groth16_params_rescale_delta step by someone who holds both sets on the device.  d = 1
 * (`after` equal to `before`) passes: that a contributor knows a d of their own is what the contribution proofs
 * (bh_pairing_same_ratio_each) establish.  With rho the coefficients expanded from seed32 (csrc/ptau_rlc.cuh) under the
 * vector tags 4 (h) and 5 (l), and x' the element of `after`, the bits of report->failed are, in the order they are
 * evaluated:
 *   SHAPE   the five queries or ic differ in length; nothing else is evaluated
 *   HEAD    delta_g1 or delta_g2 of either side is the identity or off its curve; nothing else is evaluated
 *   POINTS  only with BH_STEP_VALIDATE_POINTS in flags: h' and l' go through bh_bases_validate(CHECKED | FORBID_IDENTITY),
 *           delta_g1' and delta_g2' through the same validator; the first failure in that order ENDS the call with
 *           bad_vector (4 h, 5 l, 6 delta_g1, 7 delta_g2), bad_index and the validator's return code
 *           (BH_ERR_INVALID_POINT / BH_ERR_POINT_AT_INFINITY) - before any sum over those points is taken
 *   KEY     alpha_g1, beta_g1, beta_g2, gamma_g2 or some ic[i] differs (compared on the host): bad_vector = 0,
 *           bad_index = the position in that order (ic[i] at 4 + i)
 *   A, B_G1, B_G2   bh_bases_first_difference over the query found a difference: bad_vector = 1 / 2 / 3, bad_index = the record
 *   DELTA   e(delta_g1', delta_g2) != e(delta_g1, delta_g2')
 *   H       e(sum rho_i h_i, delta_g2) != e(sum rho_i h'_i, delta_g2'); also set when one of the two multiexps meets an
 *           identity (BH_ERR_UNEXPECTED_IDENTITY); vacuous for an empty query
 *   L       the same over l, with the coefficients of tag 5
 * The other vectors need no validation: they are compared equal to `before`'s.  bad_vector / bad_index name the FIRST
 * finding that has a position (KEY, A, B_G1, B_G2 in that order).  Returns BH_OK when failed == 0,
 * BH_ERR_INVALID_TRANSCRIPT when a bit is set, the validator's code for POINTS, call-level codes otherwise; report may be
 * NULL; an unknown flag bit is BH_ERR_INVALID_ARG.  The seed rule of bh_powers_of_tau_verify applies: seed32 MUST BE DRAWN
 * AFTER `after` IS FIXED, FROM A CSPRNG.  The four multiexps run together as ordinary jobs with the default plans (a window
 * table is used where a handle has one; none is built; each query's coefficients are expanded once and shared by both
 * sides), the up to three equations in one Miller launch.  Thread-safe (a stream of its own). */
#define BH_STEP_VALIDATE_POINTS 1u
#define BH_STEP_FAILED_SHAPE 0x001u
#define BH_STEP_FAILED_HEAD 0x002u
#define BH_STEP_FAILED_KEY 0x004u
#define BH_STEP_FAILED_A 0x008u
#define BH_STEP_FAILED_B_G1 0x010u
#define BH_STEP_FAILED_B_G2 0x020u
#define BH_STEP_FAILED_DELTA 0x040u
#define BH_STEP_FAILED_H 0x080u
#define BH_STEP_FAILED_L 0x100u
#define BH_STEP_FAILED_POINTS 0x200u
typedef struct {
  uint32_t failed;
  uint32_t bad_vector;
  size_t bad_index;
} bh_params_step_report;
int bh_groth16_params_verify_step(bh_ctx *ctx, const bh_params *before, const bh_params *after, const void *seed32,
                                  unsigned flags, bh_params_step_report *report);
/* create_proof (prover.rs:217-360) from the witness alone: input_assignment (n_inputs, [0] = 1) and
 * aux_assignment (n_aux) as produced by the circuit's alloc closures; lengths must match the R1CS. */
int bh_groth16_prove_witness(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment,
                             size_t n_inputs, const void *aux_assignment, size_t n_aux, const void *r,
                             const void *s, void *proof_out, float *timings4);
/* k proofs of ONE circuit in one call (the reference: k calls of create_proof, prover.rs:217-360): witness j =
 * (inputs + j * n_inputs * 32, aux + j * n_aux * 32), blinding (r + 32 j, s + 32 j); proofs_out + j * 384 receives
 * exactly the bytes bh_groth16_prove_witness writes for witness j (all-zero when rcs[j] != BH_OK), rcs[j] its return code:
 * BH_OK, BH_ERR_UNEXPECTED_IDENTITY (an identity delta - every proof - or an identity base met by a multiexp) or
 * BH_ERR_UNEXPECTED_EOF, with the order of reported errors per proof that the single call has.  The return value
 * carries call-level outcomes only: BH_OK, BH_ERR_INVALID_ARG (a null argument, or n_inputs / n_aux do not match the
 * R1CS: refused before anything runs), BH_ERR_DEGREE_TOO_LARGE, BH_ERR_HIP.  k = 0 is BH_OK.
 * How it runs: the proofs go through the single-proof path, at most 16 of them in flight at a time (device memory
 * stays bounded: any k is accepted), and are waited for in order.  A grouped path exists behind it (csrc/groth16.hpp,
 * BATCH_GROUPED): the five long multiexps of a group of proofs (l, a_aux, b_g1_aux, b_g2_aux, h) as five many-jobs over
 * the shared bases and densities, the h blocks one after the other on one stream, groups of g witnesses with
 * (g + 3) * m * 32 bytes <= a workspace budget of 1 GiB (m = the evaluation domain's size).  Measured against the proofs
 * in flight it is 0.51 - 1.29 x and beyond the run's own spread at two shapes of eight, other ones than in the run before
 * (profiles/prove_batch_bench.json): no basis for a rule, so this call never takes it.
 * Witness path, synchronous, one GPU; timings4 as bh_groth16_prove_witness, [1] and [2] summed over the proofs. */
int bh_groth16_prove_witness_batch(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                   const void *aux, size_t n_aux, size_t k, const void *r, const void *s, void *proofs_out,
                                   int32_t *rcs, float *timings4);
/* bh_groth16_prove_witness_batch behind a check of every witness (bh_r1cs_check_many_dev over the whole batch, in groups
 * within the workspace budget): for a witness with an unsatisfied constraint rcs[j] = BH_ERR_UNSATISFIABLE, proofs_out +
 * 384 j is all zero and first_unsatisfied[j] (k words, may be NULL) is the constraint's index; the satisfied witnesses are
 * handed to bh_groth16_prove_witness_batch's path unchanged, so every other proof is byte-identical to
 * bh_groth16_prove_witness for its witness, and its first_unsatisfied[j] is BH_R1CS_SATISFIED.  The pre-pass uploads the
 * witnesses ONCE MORE than the unchecked call (the prover uploads the satisfied ones again); its price is measured in
 * profiles/r1cs_many_bench.json.  timings4[0] = the pre-pass in host milliseconds, the rest as the unchecked call. */
int bh_groth16_prove_witness_batch_checked(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                           const void *aux, size_t n_aux, size_t k, const void *r, const void *s,
                                           void *proofs_out, int32_t *rcs, uint32_t *first_unsatisfied, float *timings4);
/* bh_groth16_prove_witness_batch / _checked over witnesses that are in DEVICE memory already - where
 * bh_r1cs_solve_many_dev left them: witness j = (inputs_dev + j * in_stride, aux_dev + j * aux_stride), layout and argument
 * checks as bh_r1cs_check_many_dev (strides in bytes, multiples of 32, at least the vector's length; BH_ERR_INVALID_ARG
 * before anything runs otherwise).  The buffers are read in place and never written, the bytes between a vector's end and
 * its stride included; nothing is uploaded.  The call waits for `stream` (the stream the caller's solve ran on; may be
 * NULL) before it reads, and drains every job before it returns.
 *   BH_PROVE_CHECK           one bh_r1cs_check_many_dev over all k on the caller's buffers first; an unsatisfied witness gets
 *                            rcs[j] = BH_ERR_UNSATISFIABLE, an all-zero slot and first_unsatisfied[j] (k words, may be NULL),
 *                            and is skipped by index - nothing is copied or compacted.  Without the bit first_unsatisfied is
 *                            not touched.
 *   BH_PROVE_FINISH_DEVICE   the proofs' tails (prover.rs:320-360) by bh_proof_finish_dev's kernels: the waited sums are laid
 *                            out k x 960 on the host and uploaded once; no blinding threads run
 *   BH_PROVE_FINISH_HOST     ... by the host arithmetic of bh_groth16_assemble, beside the GPU work
 *   neither finish bit       the measured rule (profiles/prove_batch_dev_bench.json): device finishing is ahead
 *                            of host finishing beyond its spread at three of four k = 256 shapes in every run, at the fourth in
 *                            one run of three, and at no k = 16 shape: no k qualifies and the host finishes;
 *   both                     BH_ERR_INVALID_ARG
 * proofs_out, rcs, the order of reported errors and first_unsatisfied are exactly bh_groth16_prove_witness_batch_checked's
 * (with BH_PROVE_CHECK) or bh_groth16_prove_witness_batch's on host copies of the same witnesses: every proof is
 * byte-identical to bh_groth16_prove_witness for its witness under every flag combination (prover.rs:217-360).
 * How it runs: the single-proof path, 16 proofs in flight, the multiexps and bh_r1cs_eval_dev pointed at the caller's
 * vectors.  For n_inputs <= 8 the `inputs` multiexps are answered on the host, so the input vectors (k x n_inputs x 32
 * bytes) are downloaded at the start - one copy when in_stride == n_inputs * 32, one per witness otherwise; the aux vectors
 * never leave the device.  timings4[0] = wait + check in host milliseconds, the rest as the host call. */
#define BH_PROVE_CHECK 1u
#define BH_PROVE_FINISH_DEVICE 2u
#define BH_PROVE_FINISH_HOST 4u
int bh_groth16_prove_witness_batch_dev(bh_params *params, const bh_r1cs *r1cs, const void *inputs_dev, size_t in_stride,
                                       const void *aux_dev, size_t aux_stride, size_t k, const void *r, const void *s,
                                       unsigned flags, void *stream, void *proofs_out, int32_t *rcs,
                                       uint32_t *first_unsatisfied, float *timings4);
/* ---- one caller, proofs back to back: create_proof split at the synthesis / device boundary -----------------
 * The reference's create_proof is synthesis on the host (groth16/src/prover.rs:182-215) followed by the device part
 * (:217-360); a single caller that proves in a loop leaves the GPU idle during every synthesis and the host idle during
 * every device part.  The _async calls return once the device part has been handed to a helper thread;
 * bh_groth16_proof_wait blocks for it (the Waiter of the whole proof), writes the proof and frees the job.  Issuing
 * proof k+1 before waiting for proof k overlaps its synthesis with proof k's GPU work - what groth16::ProofPipeline
 * (csrc/groth16.hpp) does for C++ callers.  Proofs are identical to the synchronous calls'.
 *   bh_groth16_prove_assignment_async  arguments as bh_groth16_prove_assignment; the arrays are READ IN PLACE until
 *                                      bh_groth16_proof_wait returns (a Rust host keeps its ProvingAssignment alive);
 *   bh_groth16_prove_witness_async     arguments as bh_groth16_prove_witness; the two witness vectors are copied before
 *                                      the call returns, the r1cs handle must outlive the wait. */
typedef struct bh_proof_job bh_proof_job;
int bh_groth16_prove_assignment_async(bh_params *params, const void *a_evals, const void *b_evals,
                                      const void *c_evals, size_t n_constraints, const void *input_assignment,
                                      size_t n_inputs, const void *aux_assignment, size_t n_aux,
                                      const uint64_t *a_aux_density, const uint64_t *b_input_density,
                                      const uint64_t *b_aux_density, const void *r, const void *s, bh_proof_job **job);
int bh_groth16_prove_witness_async(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment,
                                   size_t n_inputs, const void *aux_assignment, size_t n_aux, const void *r,
                                   const void *s, bh_proof_job **job);
int bh_groth16_proof_wait(bh_proof_job *job, void *proof_out, float *timings4);

/* ---- one proof over several GPUs: every rank holds the CRS and the matrices, builds the
 * witness and runs the (small) h block, but computes each of the eight multiexps of prover.rs:244-318
 * only over part `part` of `parts` of the scalar indices (contiguous, cut at multiples of 64).  The
 * result is BH_MSM_SUMS_BYTES = 6 x 96 + 2 x 192 bytes: affine a_inputs, a_aux, b_g1_inputs, b_g1_aux
 * (G1), b_g2_inputs, b_g2_aux (G2), h, l (G1) - the wait order of prover.rs:339-354.  The ranks
 * all-gather these records, add them slot-wise (bh_groth16_sums_add) and every rank assembles the same
 * proof (prover.rs:326-360, bh_groth16_assemble).  parts = 1 is bh_groth16_prove_witness. */
#define BH_MSM_SUMS_BYTES 960
int bh_groth16_prove_witness_part(bh_params *params, const bh_r1cs *r1cs, const void *input_assignment,
                                  size_t n_inputs, const void *aux_assignment, size_t n_aux, size_t part,
                                  size_t parts, void *sums_out, float *timings4);
void bh_groth16_sums_add(void *acc, const void *other);
int bh_groth16_assemble(bh_params *params, const void *sums, const void *r, const void *s, void *proof_out);
/* ---- k proofs from k sets of sums in one device call (prover.rs:320-360 for every proof at once) ----------------
 * bh_groth16_assemble spends five host scalar multiplications and two host linear combinations per proof; for a batch of
 * small proofs that is more than their device work.  bh_groth16_assemble_many does the same arithmetic in two kernels
 * (csrc/proof_finish.cuh): one split-scalar multiplication per (proof, product) - [r] delta1, [rs] delta1, [s] alpha1,
 * [r] beta1, [s] a_inputs, [s] a_aux, [r] b_g1_inputs, [r] b_g1_aux in G1, [s] delta2 in G2 (:326-338, 351-354) - then one
 * lane per proof element for the sums of :339-354, one inversion and the affine record.
 *   sums   k x BH_MSM_SUMS_BYTES (host), r, s   k x 32 bytes each, Montgomery (host), proofs_out   k x 384 bytes (host)
 * proofs_out + 384 j receives exactly the bytes bh_groth16_assemble(params, sums + 960 j, r + 32 j, s + 32 j, .) writes and
 * rcs[j] that call's return code: an identity delta_g1 or delta_g2 gives BH_ERR_UNEXPECTED_IDENTITY for every j
 * (prover.rs:320-324) with all-zero slots, and nothing is launched.  Returns BH_OK (k = 0 too), BH_ERR_INVALID_ARG for a
 * null argument, BH_ERR_HIP.  Synchronous; uploads k x 960 + k x 64 bytes, downloads k x 384; the verifying key's five
 * points travel as kernel arguments.  Every point must belong to the prime-order subgroup, as sums of multiples of a
 * CRS do (the split-scalar ladder is defined there only).
 * bh_proof_finish_dev is the same over device buffers: vk5 = alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2
 * (BH_FINISH_KEY_BYTES, host, bh_groth16_params_vk's order), sums_dev / r_dev / s_dev / proofs_dev laid out as above in
 * device memory, 16-byte aligned.  The kernels are enqueued on `stream` (NULL: the context's) behind whatever wrote the
 * buffers there, and the call returns once the proofs are written.  An identity delta is BH_ERR_UNEXPECTED_IDENTITY for
 * the call, before anything is launched; k = 0 is BH_OK. */
#define BH_FINISH_KEY_BYTES 672
int bh_groth16_assemble_many(bh_params *params, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                             int32_t *rcs);
int bh_proof_finish_dev(bh_ctx *ctx, const void *vk5, const void *sums_dev, const void *r_dev, const void *s_dev, size_t k,
                        void *proofs_dev, void *stream);
#ifdef __cplusplus
}
#endif
#endif
