/* libbellman_hip_test.so - self-test hooks and built-in demo circuits used by tests/, tools/ and bench.py only.  NOT part
 * of the product boundary (include/bellman_hip.h): nothing here is needed by a caller of multiexp / EvaluationDomain /
 * create_proof, and none of it is in libbellman_hip.so.  The test library links against the shipped one, so everything
 * below still runs the shipped kernels and the shipped prover (csrc/test_hooks.hip, demo_circuits.cpp,
 * groth16_callsites.cpp). */
#ifndef BELLMAN_HIP_TEST_H
#define BELLMAN_HIP_TEST_H
#include "bellman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- built-in demo circuits: create_proof on a circuit written in C++ against the mirror (like bellman user code;
 * Python cannot define one, so bench.py and the tests reach these through ctypes):
 * kind 0 = MiMCDemo (groth16/tests/common/mod.rs; witness = xl|xr, constants = `size` Fr),
 * kind 1 = synthetic multiplicative chain of `size` rounds (witness = x0),
 * kind 2 = every form of linear combination (`size` rounds, witness = x0; not satisfiable: a fixture for the host-side
 *          hooks bh_test_demo_assignment / bh_test_capture_check, bh_groth16_prove_demo rejects it),
 * kind 3 = a circuit whose structure is drawn from `seed` (`size` rounds, witness = x0; same use as kind 2),
 * kind 5 = boolean-heavy bit mixing in the shape of src/gadgets/boolean.rs (64 state bits from the low word of the witness
 *          x0, `size` AND / XOR steps, the state packed into a field element every 64 steps: > 98 % of the aux assignment
 *          is 0 or 1). */
int bh_groth16_prove_demo(bh_params *params, int circuit_kind, size_t size, uint64_t seed,
                          const void *witness, const void *constants, const void *r, const void *s,
                          void *proof_out, float *timings4);
/* the same split at the synthesis / device boundary (bh_groth16_prove_*_async of the product): synthesises the circuit
 * on the CALLING thread (prover.rs:182-215; with `r1cs` only the witness closures run, constraints are evaluated on the
 * device) and returns while the device part runs on a helper thread; bh_groth16_proof_wait collects it */
int bh_groth16_prove_demo_async(bh_params *params, const bh_r1cs *r1cs, int circuit_kind, size_t size, uint64_t seed,
                                const void *witness, const void *constants, const void *r, const void *s,
                                bh_proof_job **job);
int bh_groth16_prove_demo_r1cs_part(bh_params *params, const bh_r1cs *r1cs, int circuit_kind, size_t size,
                                    uint64_t seed, const void *witness, const void *constants, size_t part,
                                    size_t parts, void *sums_out, float *timings4);
/* The demo circuits of bh_groth16_prove_demo through that path: capture the matrices once ... */
int bh_groth16_demo_r1cs(bh_ctx *ctx, int circuit_kind, size_t size, uint64_t seed, const void *constants,
                         bh_r1cs **out);
/* ... then per proof run only the circuit's witness closures on the host (enforce is a no-op). */
int bh_groth16_prove_demo_r1cs(bh_params *params, const bh_r1cs *r1cs, int circuit_kind, size_t size,
                               uint64_t seed, const void *witness, const void *constants, const void *r,
                               const void *s, void *proof_out, float *timings4);

/* element-wise field / group ops on the device */
int bh_test_fr_mul_dev(bh_ctx *ctx, void *r_dev, const void *a_dev, const void *b_dev, size_t n);
int bh_test_fp_mul_dev(bh_ctx *ctx, void *r_dev, const void *a_dev, const void *b_dev, size_t n);
/* r[i] = a[i] + b[i] on the curve (affine in, affine out) */
int bh_test_point_add_dev(bh_ctx *ctx, int group, void *r_dev, const void *a_dev, const void *b_dev, size_t n);
/* the G2 group law in the lane-triple (K3) form of the MSM kernels (csrc/fp2k3.cuh): a[i] + b[i] by the general
 * addition, by the mixed addition (a[i] stays when b[i] is the identity), and 2 a[i]; n affine records each, HOST */
int bh_test_g2_k3_dev(bh_ctx *ctx, void *out_add_host, void *out_madd_host, void *out_dbl_host, const void *a_dev,
                      const void *b_dev, size_t n);
/* the general addition in the lane-SEXTET (K6) form of the merge kernels (csrc/msm_sums.cuh 5a): a[i] + b[i], affine out, HOST */
int bh_test_g2_k6_dev(bh_ctx *ctx, void *out_add_host, const void *a_dev, const void *b_dev, size_t n);
/* the same in the lane-pair form (csrc/fp2pair.cuh: schoolbook Fp2 products, one reduction per lane) */
int bh_test_g2_pairs_dev(bh_ctx *ctx, void *out_add_host, void *out_madd_host, void *out_dbl_host, const void *a_dev,
                         const void *b_dev, size_t n);
/* n independent pairings e(g1[i], g2[i]) (affine Montgomery records, identity = all zero), each written as 12 canonical
 * (not Montgomery) 48-byte Fp values: the w^0 .. w^5 coefficients of Fp12 = Fp2[w]/(w^6 - (u + 1)), c0 then c1 of each.
 * The value is f_{|x|,Q}(P)^(3 (p^12 - 1) / q) (csrc/fp12.cuh): oracle/pyref's pairing cubed. */
int bh_test_pairing(bh_ctx *ctx, size_t n, const void *g1_affine, const void *g2_affine, void *gt_out);
void bh_test_pairing_host(size_t n, const void *g1_affine, const void *g2_affine, void *gt_out);
/* host-side (CPU) versions of the same arithmetic headers, for toolchain-only unit tests */
void bh_test_fr_mul_host(void *r, const void *a, const void *b, size_t n);
void bh_test_fp_mul_host(void *r, const void *a, const void *b, size_t n);
void bh_test_fr_mul_bform_host(void *r, const void *a, const void *b, size_t n); /* b pre-sliced as the FFT tables are */
void bh_test_point_add_host(int group, void *r, const void *a, const void *b, size_t n);
void bh_test_point_mul_host(int group, void *r, const void *a, const void *k_canonical);
void bh_test_fr_inv_host(void *r, const void *a, size_t n); /* Montgomery in/out */
/* host only: the scalar-index slice [lo, hi) that part `part` of `parts` of a sharded proof computes */
void bh_test_proof_slice(size_t n, size_t part, size_t parts, size_t *lo, size_t *hi);
/* lazily reduced Fp helpers of the curve kernels, host build: op 0 add, 1 sub, 2 neg, 3 canonicalise,
 * 4 is_zero (returned), 5 product, 6 square, 7 eq (returned); operands are 48-byte values in [0, 2p) */
int bh_test_fp_lazy_host(int op, void *r, const void *a, const void *b);
/* host-only: milliseconds to synthesise a demo circuit (kind/size/seed as bh_groth16_prove_demo) into a
 * ProvingAssignment (mode 0) or a WitnessAssignment (mode 1); modes 2 / 3: the same into a recycled (cleared, capacity
 * kept) assignment, as create_proof does from the second proof on; no device involved */
double bh_test_synthesis_ms(int circuit_kind, size_t size, uint64_t seed, int mode);
/* host only: captures the constraint matrices of a demo circuit (what R1cs / bh_groth16_demo_r1cs does before the upload)
 * and checks them against the ProvingAssignment of the same circuit; out4 = [constraints, terms, coefficient-table
 * entries, rows that differ]; returns the capture time in ms (negative on failure) */
double bh_test_capture_check(int circuit_kind, size_t size, uint64_t seed, size_t out4[4]);
/* host only: the ProvingAssignment create_proof synthesises for a demo circuit (arguments as bh_groth16_prove_demo; input
 * constraints of prover.rs:208-215 appended).  counts3 = [n_constraints, n_inputs, n_aux]; with a == NULL only the counts
 * are returned; otherwise a, b, c (n_constraints Fr), inputs, aux (Montgomery Fr) and the three LSB0 density bitmaps */
int bh_test_demo_assignment(int circuit_kind, size_t size, uint64_t seed, const void *witness, const void *constants,
                            size_t counts3[3], void *a, void *b, void *c, void *inputs, void *aux, uint64_t *a_aux_density,
                            uint64_t *b_input_density, uint64_t *b_aux_density);
/* host build of the square roots of the compressed-point reader (csrc/point_read.cuh), n Montgomery elements (48 B in Fp,
 * c0 | c1 = 96 B in Fp2) in and out (canonical); ok[i] = 1 when a[i] is a square and r[i] one of its roots, else 0 */
void bh_test_fp_sqrt_host(void *r, unsigned char *ok, const void *a, size_t n);
void bh_test_fp2_sqrt_host(void *r, unsigned char *ok, const void *a, size_t n);
void bh_test_fr_from_u512_host(void *r, const void *limbs8); /* 64 bytes LE -> Montgomery Fr (create_random_proof's sampling) */
/* host only: the scalar-field arithmetic of the C++ mirror (bellman::Fr, csrc/groth16.hpp - what circuits and the
 * linear-combination evaluation compute with during synthesis), n operations on arrays of 32-byte Montgomery elements:
 * op 0 r = a + b, 1 r = a - b, 2 r = a * b (b may be ANY 256-bit value), 3 r = -a, 4 r = Fr::from_u64(low limb of a),
 * 5 r = canonical limbs of a (to_canonical), 6 r = a^-1 (a != 0) */
void bh_test_fr_ops_host(int op, void *r, const void *a, const void *b, size_t n);

/* ONE field operation per element on operands of the caller's choice, raw results (nothing is canonicalised), through the
 * function objects the kernels use (csrc/test_field_hooks.hip; tests/test_gpu_field_corners.py).  Operands and results
 * are arrays of fixed-size slots; flags[k] carries a predicate's answer (0 elsewhere).
 *   form 0 / 1  canonical Fe<FrParams> / Fe<FpParams> (32 / 48-byte slots): op 0 fe_add, 1 fe_sub, 2 fe_neg, 3 fe_dbl,
 *               4 fe_mul, 5 fe_mul_b(a, fe_to_bform(b)), 6 fe_sqr, 7 fe_to_mont, 8 fe_from_mont, 9 fe_inv
 *   form 2 / 3  FpOps / Fp2Ops, lazily reduced (48 / 96-byte slots): op 0 add, 1 sub, 2 neg, 3 dbl, 4 canon, 5 is_zero,
 *               6 eq, 7 mul, 8 mul_tail, 9 sqr, 10 mul2_sub(a, b, c, d), 11 mul2_sub_tail, 12 inv; form 2 only:
 *               13 fpl_add2, 14 fpl_sub2 on the pairs (a, b) and (c, d): two results per element
 *   form 4 / 5  Fp2K3Ops / Fp2PairOps (device only; 96-byte Fp2 operands, the kernels' lane mapping): the ops of form 3
 *               up to 7, 9, and 13 load / store round trip, 14 one, 15 curve_b.  r = n * LANES 48-byte lane values (what
 *               lane `role` of element i holds: r[i * LANES + role], the sum lane of a triple included) followed by the n
 *               Fp2 values F::store wrote; flags[i * LANES + role]
 *   form 6      the tower of csrc/fp12.cuh, 576-byte slots (an operation reads as much of a slot as its argument type
 *               needs): op 0 f2_mul_xi, 1 f2_mul_fp(a, b: Fp), 2 f2_conj, 3 / 4 / 5 f2_mul_small by 3 / 4 / 12, 6 f6_mul,
 *               7 f6_mul_01(a, b, c), 8 f6_mul_1(a, b), 9 f6_mul_v, 10 f6_inv, 11 f12_mul, 12 f12_sqr,
 *               13 f12_mul_line(a; b, c, d), 14 f12_inv, 15 f12_conj, 16 f12_frob1, 17 f12_frob2, 18 f12_cyc_sqr,
 *               19 f12_cyc_exp_x, 20 f12_is_one (flag), 21 f12_final_exp (canonical, flag = is one); on the device 19
 *               and 21 are the kernel chains of csrc/final_exp.cuh
 *   form 7      csrc/point_read.cuh, 96-byte slots: op 0 fp_sqrt (c0; flag = ok), 1 fp2_sqrt (flag = ok), 2 fpl_half (c0),
 *               3 fp_lex_largest (c0; flag), 4 fp2_lex_largest (flag)
 * bh_test_field_ops_shape: out4 = [result bytes per element, flags per element, operand slot bytes, operands used]. */
int bh_test_field_ops_shape(int form, int op, size_t out4[4]);
int bh_test_field_ops_dev(bh_ctx *ctx, int form, int op, void *r_dev, uint32_t *flags_dev, const void *a_dev,
                          const void *b_dev, const void *c_dev, const void *d_dev, size_t n);
/* the same `apply` compiled for the host (forms 0 - 3, 6, 7) */
int bh_test_field_ops_host(int form, int op, void *r, uint32_t *flags, const void *a, const void *b, const void *c,
                           const void *d, size_t n);

/* ONE group operation per worker on RAW projective operands of the caller's choice, raw results (nothing is canonicalised),
 * through the functions the kernels call and with the kernels' worker and lane mapping (csrc/test_group_hooks.hip;
 * tests/test_gpu_group_law.py, tests/test_group_model_cpu.py).  Records are XYZZ<Mem> (X, Y, ZZ, ZZZ: 4 x 48 bytes in G1,
 * 4 x 96 in G2, every coordinate a Montgomery residue in [0, 2p)) and canonical affine records (x, y; all zero = identity).
 *   form 0  G1, one lane (XYZZ<FpOps>)            device and host
 *   form 1  G1, lane pairs (HalfWorker<PairHalf>)    device
 *   form 2  G2, one lane (Fp2Ops)                 device and host
 *   form 3  G2, lane triples (Fp2K3Ops)           device
 *   form 4  G2, lane pairs (Fp2PairOps)           device
 *   form 5  G2, lane sextets (HalfWorker<SextetHalf>) device
 *   op  0 add            r = a + b: xyzz_add (forms 0, 2, 3, 4), half_add (1, 5); b = XYZZ records
 *       1 add_alias      the same with r aliasing a, as the merge kernels call it
 *       2 madd           r = a + b, b = AFFINE records: xyzz_madd; an identity b is skipped as the accumulation does
 *       3 madd_prefetch  the overload with a prefetch functor, which loads the first word of b's record
 *       4 dbl            xyzz_dbl(a)
 *       5 dbl_affine     xyzz_dbl_affine(b), b affine and not the identity
 *       6 from_affine    xyzz_from_affine(b)
 *       7 to_affine      xyzz_to_affine(a) into X, Y of the result (ZZ = ZZZ = 0); forms 0 and 2 only: the lane bundles
 *                        have no inversion, and no kernel converts in those forms
 *       8 is_identity    xyzz_is_identity(a); r = a
 *       9 load_store     PairHalf / SextetHalf load and store, round trip (forms 1 and 5 only)
 *      10 tree           r[g] = a[g G] + ... + a[g G + G - 1] by group_reduce_points / half_group_reduce (WK::tree) over
 *                        G consecutive workers of a wavefront, G a power of two in [2, workers per wavefront]; n groups
 *      11 block_sum      r[c] = the sum of the 4 x (workers per wavefront) records of case c by long_block_sum at
 *                        LONG_THREADS, one workgroup per case; on the host G = the workers per wavefront to fold by
 *                        (0: the form's own), so that a host run adds in the order of any device form of the same group
 *   ops 2 - 8 exist for forms 0, 2, 3, 4.  flags: `lanes` words per worker, one per lane of the worker (flags[i * lanes +
 *   role]): bit 0 = the result is the identity as the form's own predicate sees it in that lane (to_affine: the affine
 *   record is the identity), bit 1 = what xyzz_madd returned, bits 4-7 = how often the prefetch functor ran, bits 16-31 =
 *   the low half of the word it loaded.
 * bh_test_group_ops_shape: out4 = [XYZZ record bytes, flag words per worker, affine record bytes, workers per wavefront
 * in the trees]. */
int bh_test_group_ops_shape(int form, int op, size_t out4[4]);
int bh_test_group_ops_dev(bh_ctx *ctx, int form, int op, unsigned G, void *r_dev, uint32_t *flags_dev, const void *a_dev,
                          const void *b_dev, size_t n);
/* the same `apply` compiled for the host (forms 0 and 2); trees and block sums add in the order of the shuffle trees */
int bh_test_group_ops_host(int form, int op, unsigned G, void *r, uint32_t *flags, const void *a, const void *b, size_t n);
/* msm_sum_kernel on its own: up to three reduction jobs in ONE launch, counted and launched by sum_launch as msm_enqueue
 * does.  form = the worker kind (the forms above; 4 has no sum kernel), waves = wavefronts per workgroup:
 *   (0, 1) one-lane G1   (1, 1) lane pairs   (1, 2), (1, 4) lane pairs, "wide"   (2, 1) one-lane G2 (LDS accumulators)
 *   (3, 4) lane triples   (5, 4) lane sextets
 * in_dev: n_in XYZZ records, out_dev: n_out.  A job is 11 words - mode (1 strided, 2 bits), groups, count, inner, stride,
 * istride, group_shift, splits, lanes (a power of two <= waves x workers per wavefront in the trees), and the record
 * offsets of its input and output - SumDesc of csrc/msm_types.hpp; a job that would read or write outside the buffers
 * is refused.  out[out_off + g], g < groups, are the raw sums. */
int bh_test_sum_jobs_dev(bh_ctx *ctx, int form, unsigned waves, const void *in_dev, size_t n_in, void *out_dev, size_t n_out,
                         const uint32_t *jobs, size_t n_jobs);

/* The mixed addition of the G1 bucket accumulation over sliced operands (csrc/test_sliced_hooks.hip, ec.cuh
 * xyzz_madd_sliced; tests/test_gpu_madd_sliced.py) next to xyzz_madd: a = n raw XYZZ records, q = n affine records (G1, one
 * lane).  r = 2 n raw records: r[i] xyzz_madd(a[i], q[i]), r[n + i] the sliced addition.  An identity q[i] is skipped as the
 * accumulation skips it.  flags[i]: bit 0 what xyzz_madd returned, bit 1 what the sliced addition returned, bit 4 q[i] was
 * the identity. */
int bh_test_g1_madd_sliced_dev(bh_ctx *ctx, void *r_dev, uint32_t *flags_dev, const void *a_dev, const void *q_dev, size_t n);
int bh_test_g1_madd_sliced_host(void *r, uint32_t *flags, const void *a, const void *q, size_t n);

/* Stage 4 of a multiexp on its own (csrc/test_bucket_hooks.hip; tests/test_gpu_bucket_stage.py, tests/models/
 * bucket_stage_model.py): msm_accumulate_kernel, msm_merge_chunks_kernel and the tail - msm_merge_tail_kernel, or
 * msm_merge_runs_kernel + msm_merge_long_kernel - over a SORTED pair stream of the caller's choice, launched by the functions
 * msm_enqueue launches them with (launch_accumulate, launch_merges of csrc/msm_ec.cuh), with the merge parameters of the
 * shipped merge_plan and queues sized by the shipped merge_bounds.
 *   acc_form    0 G1 in registers   1 G1, accumulator in LDS   2 G2 one lane, accumulator in LDS (pipelined)
 *               3 G2 one lane in registers (pipelined)   4 G2 lane triples   5 G2 lane pairs
 *   merge_form  0 G1, medium runs on XyzzWorker<FpOps>   1 G1, medium runs on lane pairs (big runs: lane pairs in both)
 *               2 G2 in lane triples, medium runs on XyzzWorker<Fp2K3Ops>   3 ... on lane sextets (big runs: sextets in both)
 *               4 G2 one lane, the fused tail kernel (needs W 2^(c-1) > 128 buckets)   5 G2 one lane, the two launches
 *               (needs at most 128 buckets)
 * bh_test_bucket_stage_shape: out12 = [XYZZ record bytes, dense affine record bytes, partials per piece, workers per
 * wavefront of the medium worker, ... of the big worker, smallest and largest admissible G (workers per medium run, a
 * power of two), guard bytes behind every returned buffer, sizeof LongRun, BigRun, ErrFlags, the sentinel byte].
 * bh_test_merge_plan (host only): the merge parameters of a plan (W windows of n entries, c window bits, chunks of K,
 * chunks_per_window lanes per window; NB = W 2^(c-1), nb = 2^(c-1)) on a chip of num_cus compute units: plan_out8 = [walk,
 * run_lanes (G), runs_on_pairs, big_chunks, piece, max_long, max_big, max_pieces].  The form fixes which worker folds the medium
 * runs; where merge_plan chose the other one G is 8.  Here alone merge_form may also be 6, 7 or 8: the plan of the bundle FpOps,
 * Fp2K3Ops or Fp2Ops exactly as msm_enqueue gets it.  overrides4 (optional; 0 = keep) = [walk, run_lanes, big_chunks, block
 * cap]: the bounds are then the shipped bounds of the overridden values.  block cap b: at most b workgroups for the medium
 * runs and 2 b for the pieces of the big runs.
 * bh_test_bucket_stage_dev: pairs = W x n entries (|digit| << 32 | sign << 31 | base index), zstart[W] = each window's first
 * live entry, bases = n_bases affine records base_stride bytes apart (the dense size; 128 with acc_form 0).  Refused before
 * any launch: live digits that decrease or leave [1, 2^(c-1)], a base index >= n_bases, z > n, n > chunks_per_window K, a G
 * that is no power of two in the admissible range, W > 16, n > 2^20, c > 16, more than 2^20 chunks.  With every output pointer
 * NULL it only fills plan_out8: the caller sizes its buffers by it - pts_out W 2^(c-1) records, head_out and tail_out
 * W chunks_per_window records, long_out max_long LongRun, big_out max_big BigRun, pieces_out max_pieces records, err_out one
 * ErrFlags, each followed by the guard bytes - and calls again.  pts and ErrFlags start zeroed as in production; head,
 * tail, the piece results, both queues and every guard start filled with the sentinel byte. */
int bh_test_bucket_stage_shape(int acc_form, int merge_form, size_t out12[12]);
int bh_test_merge_plan(int merge_form, unsigned W, unsigned n, unsigned c, unsigned K, unsigned chunks_per_window, int num_cus,
                       const uint32_t *overrides4, uint32_t plan_out8[8]);
int bh_test_bucket_stage_dev(bh_ctx *ctx, int acc_form, int merge_form, const uint64_t *pairs, const uint32_t *zstart, unsigned W,
                             unsigned n, const void *bases, size_t n_bases, unsigned base_stride, unsigned c, unsigned K,
                             unsigned chunks_per_window, const uint32_t *overrides4, uint32_t plan_out8[8], void *pts_out,
                             void *head_out, void *tail_out, void *long_out, void *big_out, void *pieces_out, void *err_out);
/* Which of a base handle's sources a multiexp reads (csrc/msm_types.hpp msm_pick_sources; tests/test_msm_sources_cpu.py).
 * Host only: the views' pointers are tags.  table_kind: 0 no window table, 1 one at the dense record stride (96 / 192
 * bytes), 2 one at a 128-byte stride; tab_c, tab_W, tab_row_records describe it (window bits, rows, records per row);
 * has_padded: the vector has a copy at a 128-byte stride; flags, opts_c: bh_msm_opts; n scalars; acc_form: 0 one lane per
 * point with the accumulator in registers, 1 ... in LDS, 2 several lanes per point.  out6 = [use_table, the view the
 * accumulation gathers from (0 the vector, 1 its padded copy, 2 the table), its stride in bytes, the view the
 * error-resolution pass reads, its stride, 1 where the source allows the one-launch small path].  BH_ERR_INVALID_ARG for a
 * layout no kernel reads (a G2 table at 128 bytes). */
int bh_test_msm_sources(int group, int table_kind, int has_padded, uint32_t flags, unsigned opts_c, unsigned tab_c, unsigned tab_W,
                        uint64_t tab_row_records, uint64_t n, int acc_form, uint32_t out6[6]);
/* window_table_kernel on its own (tests/test_gpu_window_table_build.py): the table of n <= 4096 affine records, rows of c
 * window bits, built by the function bh_bases_precompute builds it with into a buffer of ceil(256 / c) n `stride` bytes
 * filled with the sentinel byte and followed by the guard (bh_test_bucket_stage_shape); table_out receives both raw.
 * stride: 96 or 128 (G1), 192 (G2); any other is refused. */
int bh_test_window_table_dev(bh_ctx *ctx, int group, const void *points, size_t n, unsigned stride, unsigned c, void *table_out);

/* Stage 5 of a multiexp on its own, and its host tail (csrc/test_reduce_hooks.hip; tests/test_gpu_reduce_stage.py,
 * tests/models/reduce_stage_model.py): the row / column sums, their two-stage split over piece sums, the bit sums and the
 * window totals over FILLED BUCKETS of the caller's choice, issued by the function msm_enqueue issues them with
 * (launch_reduce of csrc/msm_ec.cuh) into buffers of exactly the sizes msm_enqueue carves (reduce_plan of
 * csrc/msm_stage_plans.hpp).
 *   form   0 G1 (FpOps)   1 G2 on lane triples (Fp2K3Ops)   2 G2 one lane (Fp2Ops): the bundles msm_enqueue reduces with
 *   kind   0 the classic plan (make_plan: W = ceil(256 / c) windows)   1 the table plan (make_table_plan: W = 1)
 *   c      window bits, 2 ... 24.  num_cus: 0 = the context's own, else passed to the plan in its place (it steers choices
 *          only; grids come from the descriptors)
 * bh_test_reduce_plan (host only; ctx may be NULL unless num_cus is 0): plan_out16 = [c, W, nb, NB, lo_bits, hi_bits, two_len,
 * want_part, records of rowcol, of part, of bits, guard bytes, the sentinel byte, XYZZ record bytes, affine record bytes,
 * num_cus used].  *n_launches_out = the launches launch_reduce issues, in order - the schedule of the plan that reduce_plan
 * returns, which is all launch_reduce reads; launches_out (optional, room for max_launches) = 46 words each:
 * [worker kind (the forms of bh_test_sum_jobs_dev), wavefronts per workgroup, workgroups, lanes a workgroup holds], then three
 * jobs of 14 words: the 11 of bh_test_sum_jobs_dev after sum_count's clamping, with offsets in records inside the job's
 * buffers, then [buffer read, buffer written, workgroups]; buffers 0 pts, 1 rowcol (rows, then cols at W 2^hi_bits), 2 part,
 * 3 bits.  A job with groups = 0 does nothing; launches of no workgroup are not part of the plan.
 * bh_test_reduce_stage_dev: pts_in = NB raw XYZZ records.  rowcol, part and bits are allocated at exactly the planned sizes,
 * each followed by a guard; bits starts zeroed as in production, rowcol, part and every guard filled with the sentinel byte.
 * launch_reduce runs once on the context's stream; rowcol_out, part_out, bits_out receive the buffers raw (part_out may not be
 * NULL even where the plan has no part); guards_out4 = [pts, rowcol, part, bits]: 1 = the guard came back untouched (pts: and
 * the buckets themselves unchanged).  affine_out = the shipped msm_host_tail over bits_out.  Refused before any launch: c
 * outside [2, 24], a form or kind that does not exist, NB above 2^22 records, a recorded launch that would leave its buffers.
 * bh_test_msm_host_tail (host only): msm_host_tail<FpOps> (group 1) / <Fp2Ops> (group 2) over W c raw records of the
 * caller's choice in the layout of bits - [W][lo_bits] column-bit sums, [W][hi_bits] row-bit sums, [W] totals - for the
 * plan (kind, c). */
int bh_test_reduce_plan(bh_ctx *ctx, int form, int kind, unsigned c, int num_cus, uint32_t plan_out16[16], uint32_t *launches_out,
                        size_t max_launches, size_t *n_launches_out);
int bh_test_reduce_stage_dev(bh_ctx *ctx, int form, int kind, unsigned c, int num_cus, const void *pts_in, void *rowcol_out,
                             void *part_out, void *bits_out, uint32_t guards_out4[4], void *affine_out);
int bh_test_msm_host_tail(int group, int kind, unsigned c, const void *bits_in, void *affine_out);

/* Stages 1 - 3 of a multiexp on their own (csrc/test_sort_hooks.hip, which compiles csrc/msm_stages.hip a second time into
 * the test library; tests/test_gpu_sort_stage.py, tests/models/sort_stage_model.py): density prefix, recursive scan,
 * signed-digit recoding, the 8-bit sort of the classic plan, the fused recode-and-sort of the table plan, the zero-digit search.
 * kind: 0 the classic plan (make_plan; n entries per window, stride must be 0), 1 the table plan (make_table_plan over a table
 * of ceil(256/c) rows `stride` records apart; n scalars).  Refused everywhere: c outside [2, 24], n = 0, Wd n >= 2^32,
 * Wd stride >= 2^31 - the conditions of msm_enqueue.
 * bh_test_sort_plan (host only): plan_out23 = [n, c, W, nd, Wd, num_tiles, sort_passes, base_stride, key bits of passes 0 - 3
 * (0 where there is no such pass), wide_scalars_per_tile and the first pass's tile count (table plan; else 0),
 * sort_counts_elems, scan_tmp_elems(counts + 1), SORT_TILE, WIDE_TILE, WIDE_THREADS, SCAN_TILE, guard bytes, the sentinel
 * byte, sizeof ErrFlags].
 * bh_test_scan_dev: exclusive_scan_u32 in place over data[n] (n <= 2^24) with a scratch of exactly scan_tmp_elems(n) words,
 * which is returned raw in tmp_out; *tmp_elems_out is that count, and with data, tmp_out and guards_out2 all NULL nothing
 * else happens (host only: ctx may be NULL, any n < 2^32).  guards_out2 = [data, scratch]: 1 when the guard bytes behind the buffer came back untouched.
 * bh_test_sort_stage_dev: msm_run_stages once, on the context's stream, over nd scalars (32 bytes each; Montgomery ones must
 * be below q) and an optional density bitmap of ceil(nd / 64) words; at most 2^21 entries (Wd nd).  Buffers as msm_enqueue
 * sizes them, without its rounding to 256 bytes: pairs_a_out and pairs_b_out Wd nd entries, zstart_out W words, counts_out
 * sort_counts_elems + 1, word_prefix_out ceil(nd / 64) + 1 (NULL exactly when density_words is), err_out one ErrFlags.
 * ErrFlags starts zeroed as in production, everything else and every guard filled with the sentinel byte.
 * *sorted_is_b_out: which pair array msm_run_stages returned.  guards_out8 = [pairs_a, pairs_b, counts, scan scratch, zstart,
 * word_prefix, ErrFlags, scalars]: 1 = untouched. */
int bh_test_sort_plan(int kind, size_t n, unsigned c, size_t stride, int g2, int num_cus, uint64_t plan_out23[23]);
int bh_test_scan_dev(bh_ctx *ctx, uint32_t *data, size_t n, size_t *tmp_elems_out, uint32_t *tmp_out, uint32_t guards_out2[2]);
int bh_test_sort_stage_dev(bh_ctx *ctx, int kind, unsigned c, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                           size_t skip, size_t n_bases, size_t stride, uint64_t *pairs_a_out, uint64_t *pairs_b_out,
                           int *sorted_is_b_out, uint32_t *zstart_out, uint32_t *counts_out, uint32_t *word_prefix_out, void *err_out,
                           uint32_t guards_out8[8]);

/* The one-launch small path and the error-resolution pass on their own (csrc/test_small_hooks.hip; tests/test_gpu_small_fill.py,
 * tests/test_small_fill_model_cpu.py, tests/models/small_fill_model.py): msm_small_fill_kernel - signed digits, density rank,
 * EOF rule, per-bucket entry lists and their table-scan fallback, four workers per bucket - which replaces stages 1 - 4 of a
 * small multiexp over a window table, launched by the function msm_enqueue launches it with (launch_small_fill of
 * csrc/msm_ec.cuh) as the shipped plans say (make_table_plan; small_fill_plan of csrc/msm_stage_plans.hpp, which holds the gate
 * that chooses the path); and msm_err_resolve_kernel, launched as msm_finish launches it (err_resolve_lo_ref, launch_err_resolve).
 *   form   0 FpOps (G1)   1 Fp2K3Ops (G2, lane triples)   2 Fp2PairOps (G2, lane pairs)   3 Fp2Ops (G2, one lane)
 * A table: ceil(256 / c) rows of row_records affine records at the dense stride (96 / 192 bytes), row w at w row_records.
 * Refused everywhere: a form that does not exist, nd = 0, c outside [2, 24], Wd nd >= 2^32, Wd row_records >= 2^31 - the
 * conditions of msm_enqueue and msm_pick_sources.
 * bh_test_small_fill_plan (host only): the plans of nd scalars over such a table with the option flags `flags` (bh_msm_opts):
 * plan_out20 = [fused, workgroups, threads, dynamic LDS bytes, buckets per workgroup, top_bits, sliver_load, Wd, entries (Wd nd),
 * nb (2^(c-1) buckets), SMALL_MAX_SCALARS, SMALL_MAX_ENTRIES, SMALL_MAX_PER_BUCKET, SMALL_LIST_CAP, SMALL_LANES_PER_BUCKET, XYZZ
 * record bytes, affine record bytes, guard bytes, the sentinel byte, sizeof ErrFlags].
 * bh_test_small_fill_dev: launch_small_fill once, on the context's stream, over nd scalars (32 bytes each; Montgomery ones
 * must be below q), an optional density bitmap of ceil(nd / 64) words, skip, n_bases, and table = Wd row_records affine
 * records.  Buffers as msm_enqueue carves them, without its rounding to 256 bytes: pts_out nb XYZZ records and err_out one
 * ErrFlags, both zeroed as in production; word_prefix_out ceil(nd / 64) + 1 words, filled with the sentinel byte, passed to the
 * kernel - and wanted here - exactly when density_words is given.  All three come back raw.  guards_out6 = [pts, word_prefix,
 * ErrFlags, scalars, density, table]: 1 = the guard bytes behind the buffer came back untouched.  Refused before any launch: a
 * shape the shipped plan does not fuse, n_bases > row_records (a live scalar's base cursor is below n_bases: inside a row),
 * row_records > 2^16, skip >= 2^31, a scalar format that does not exist, a Montgomery scalar >= q.
 * bh_test_err_resolve_lo_ref (host only): err_resolve_lo_ref(nref), the first bit of the reference's top window over nref
 * exponents.
 * bh_test_err_resolve_dev: launch_err_resolve once over nd <= 2^20 scalars, an optional density bitmap WITH its word prefix
 * (ceil(nd / 64) + 1 words, the caller's), skip, n_bases, bases = n_records affine records of group 1 / 2 base_stride bytes apart
 * (n_bases <= n_records <= 2^20: what lies behind n_bases is there to be left alone; strides 96 or 128 in G1, 192 in G2, any other
 * is refused) and the top window of ref_n exponents (0: of nd, as msm_finish takes it).  err_inout: one ErrFlags, uploaded as the
 * caller set it and returned raw.  guards_out5 = [scalars, density, word_prefix, bases, ErrFlags]. */
int bh_test_small_fill_plan(int form, size_t nd, unsigned c, size_t row_records, uint32_t flags, uint64_t plan_out20[20]);
int bh_test_small_fill_dev(bh_ctx *ctx, int form, unsigned c, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                           size_t skip, size_t n_bases, const void *table, size_t row_records, void *pts_out,
                           uint32_t *word_prefix_out, void *err_out, uint32_t guards_out6[6]);
uint32_t bh_test_err_resolve_lo_ref(uint64_t nref);
int bh_test_err_resolve_dev(bh_ctx *ctx, int group, const void *scalars, int fmt, size_t nd, const uint64_t *density_words,
                            const uint32_t *word_prefix, size_t skip, size_t n_bases, const void *bases, size_t n_records,
                            unsigned base_stride, uint64_t ref_n, void *err_inout, uint32_t guards_out5[5]);

/* The kernels of the Groth16 verifier on their own (csrc/test_pairing_hooks.hip, which compiles csrc/pairing_kernels.cuh a
 * second time into the test library; tests/test_gpu_pairing_stages.py, tests/models/pairing_stage_model.py).  Each call runs
 * one stage once on the context's stream through the shipped launch function (launch_g2_lines, launch_miller, launch_fold,
 * launch_colsum, launch_fold3_const, launch_final_exp) or, where the verifier launches the kernel inline, with the verifier's
 * block size.  Every device buffer has exactly the size the verifier gives it for n proofs, followed by a guard; outputs
 * and guards start filled with the sentinel byte, results come back raw, and guards[k] = 1 when the guard behind buffer k
 * (in the order given below) came back untouched.  Refused before any launch: n = 0 or n > 2^15, a width outside
 * {1, 2, 4, 8}, a stride other than 192 or 384, nb_override > COLSUM_BLOCKS, a scalar format that does not exist.
 * bh_test_pairing_stage_shape: out16 = [sizeof line_t, fp12_t, ProofRec, MILLER_LINES, PF_IDENTITY, PF_OFF_CURVE,
 *   PT_INVALID_MASK, PT_IS_INF, COLSUM_THREADS, COLSUM_BLOCKS, BATCH_CHUNK, guard bytes, the sentinel byte, the offsets of
 *   ProofRec::b and ::c, sizeof an affine G1 record].
 * lines: n records stride_bytes apart (192: G2 points; 384: proofs, the point at ProofRec::b); lines_out n x 68 line_t,
 *   flags_out n words.  guards: [records, lines, flags].
 * miller: p = n0 + n1 G1 points; lines0 / flags0 serve the first n0, lines1 / flags1 the rest.  guards: [p, lines0, flags0,
 *   lines1, flags1, f].
 * fold: launch_fold over f_inout[m]; the whole array comes back.
 * proof_prep: z may be NULL; want_c = 0 passes NULL for c_out, zc_out and the generator.  guards: [proofs, z, generator,
 *   p_out, c_out, zc_out, flags].
 * g1_mul_one: guards [p, s, out].
 * colsum: launch_colsum over n proofs of n_inputs inputs each; acc_inout n_inputs + 1 values (read and written), part_out
 *   (n_inputs + 1) x COLSUM_BLOCKS values; nb_override 0 = the shipped rule.  guards: [z, inputs, part, acc].
 * ic_table: the (n_in, 256 / w, 2^w - 1) table of ic[n_in].  guards: [ic, table].
 * ic_accumulate: over a table of the caller's (n_inputs = 0: table may be NULL).  guards: [inputs, table, ic0, out].
 * miller3: separate != 0: gridDim.y = 3 and f_out 3 n values (pairs is then ignored); else gridDim.y = 1, f_out n values.
 *   klines 2 x 68 lines, kflags2 2 words.  guards: [a, acc, proofs, blines, bflags, klines, kflags, f].
 * fold3_const: launch_fold3_const over f_inout (3 n values when separate, else n) and the constant c.  guards: [f, c].
 * verdict: words may be NULL.  guards: [words, pflags, qflags, is_one, verdicts].
 * final_exp: launch_final_exp over n <= 4096 values with a workspace of 4 n.  guards: [f, out, is_one, workspace]. */
int bh_test_pairing_stage_shape(uint64_t out16[16]);
/* host only: the verifier's proof_status_error of a status word of bh_proofs_read */
int bh_test_proof_status_error(uint32_t word);
int bh_test_pairing_lines_dev(bh_ctx *ctx, const void *records, size_t stride_bytes, int negate, size_t n, void *lines_out,
                              uint32_t *flags_out, uint32_t guards[3]);
int bh_test_pairing_miller_dev(bh_ctx *ctx, const void *p, const void *lines0, const uint32_t *flags0, size_t n0,
                               const void *lines1, const uint32_t *flags1, size_t n1, void *f_out, uint32_t guards[6]);
int bh_test_pairing_fold_dev(bh_ctx *ctx, void *f_inout, size_t m, uint32_t guards[1]);
int bh_test_pairing_proof_prep_dev(bh_ctx *ctx, const void *proofs, const void *z, int fmt, size_t n, int want_c,
                                   const void *g1_generator, void *p_out, void *c_out, void *zc_out, uint32_t *flags_out,
                                   uint32_t guards[7]);
int bh_test_pairing_g1_mul_one_dev(bh_ctx *ctx, const void *p, const void *s_mont, void *out, uint32_t guards[3]);
int bh_test_pairing_colsum_dev(bh_ctx *ctx, const void *z, const void *inputs, size_t n_inputs, int fmt, size_t n,
                               unsigned nb_override, void *acc_inout, void *part_out, uint32_t guards[4]);
int bh_test_pairing_ic_table_dev(bh_ctx *ctx, const void *ic, size_t n_in, unsigned w, void *table_out, uint32_t guards[2]);
int bh_test_pairing_ic_accumulate_dev(bh_ctx *ctx, const void *inputs, size_t n_inputs, int fmt, const void *table, unsigned w,
                                      const void *ic0, size_t n, void *out, uint32_t guards[4]);
int bh_test_pairing_miller3_dev(bh_ctx *ctx, const void *a, const void *acc, const void *proofs, const void *blines,
                                const uint32_t *bflags, const void *klines, const uint32_t *kflags2, int separate, unsigned pairs,
                                size_t n, void *f_out, uint32_t guards[8]);
int bh_test_pairing_fold3_const_dev(bh_ctx *ctx, void *f_inout, const void *c, size_t n, int separate, uint32_t guards[2]);
int bh_test_pairing_verdict_dev(bh_ctx *ctx, const uint32_t *words, const uint32_t *pflags, const uint32_t *qflags,
                                const uint32_t *is_one, size_t n, int32_t *verdicts_out, uint32_t guards[5]);
int bh_test_pairing_final_exp_dev(bh_ctx *ctx, const void *f, size_t n, void *out, uint32_t *is_one_out, uint32_t guards[4]);
/* The key-aware kernels of the calls over a bh_pvk_set, each through its launch function (launch_ic_accumulate_keys,
 * launch_miller3_keys, launch_fold3_const_keys, launch_colsum_keys, launch_g1_mul_keys, launch_miller_keys;
 * tests/test_gpu_verify_keys_stages.py).  bh_test_key_layout names the keys: n_inputs and widths (1, 2, 4, 8) per key, the
 * keys' window tables one after another (key k: n_inputs[k] x 256 / w x (2^w - 1) records), and per key ic_0, the 3 x 68
 * lines of -gamma, -delta, beta with their 3 flag words, f(-alpha, beta) and alpha; an array that the kernel of a hook does
 * not read may be NULL.  The hook uploads them as seven buffers - tables, ic_0, lines, flags, f(-alpha, beta), alpha,
 * descriptors - whose guards FOLLOW the hook's own in `guards`, and writes the descriptor table (column offsets: the keys'
 * n_inputs + 1 columns side by side) before the launch.  blocks: nblocks x {key, first row, row count 1 .. 64, first
 * scalar}; segs: n_keys x {first row, row count, first scalar, 0}.  Refused before any launch: a key, row or scalar out of
 * range in blocks or segs, more than 64 keys or inputs per key, an array that the kernel reads left NULL.
 * ic_accumulate_keys: inputs n_scalars values, out n records.  guards: [inputs, blocks, out] + 7.
 * miller3_keys: as miller3 with pairs = 7.  guards: [a, acc, proofs, blines, bflags, blocks, f] + 7.
 * fold3_const_keys: guards [f, blocks] + 7.
 * colsum_keys: acc_inout and part_out hold the set's total columns (x COLSUM_BLOCKS for part).  guards: [z, inputs, segs,
 *   part, acc] + 7.
 * g1_mul_keys: out[k] = [acc_mont[column offset of k]] alpha_k.  guards: [acc, out] + 7.
 * miller_keys: p and f_out 3 n_keys values, [which][key].  guards: [p, f] + 7. */
typedef struct bh_test_key_layout {
  size_t n_keys;
  const uint32_t *n_inputs;
  const uint32_t *widths;
  const void *tables;
  const void *ic0;
  const void *lines;
  const uint32_t *qflags;
  const void *f_ab;
  const void *alpha;
} bh_test_key_layout;
int bh_test_pairing_ic_accumulate_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                           const void *inputs, size_t n_scalars, int fmt, size_t n, void *out, uint32_t guards[10]);
int bh_test_pairing_miller3_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                     const void *a, const void *acc, const void *proofs, const void *blines,
                                     const uint32_t *bflags, int separate, size_t n, void *f_out, uint32_t guards[14]);
int bh_test_pairing_fold3_const_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *blocks, size_t nblocks,
                                         void *f_inout, size_t n, int separate, uint32_t guards[9]);
int bh_test_pairing_colsum_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const uint32_t *segs, const void *z,
                                    const void *inputs, size_t n_scalars, int fmt, size_t n, unsigned nb_override, void *acc_inout,
                                    void *part_out, uint32_t guards[12]);
int bh_test_pairing_g1_mul_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const void *acc_mont, void *out,
                                    uint32_t guards[9]);
int bh_test_pairing_miller_keys_dev(bh_ctx *ctx, const bh_test_key_layout *keys, const void *p, void *f_out, uint32_t guards[9]);

/* ---- the powers-of-tau check (csrc/ptau_rlc.cuh, compiled into this library by csrc/test_ceremony_hooks.hip) -----------
 * bh_test_ptau_rlc_host / _dev: the `count` coefficients of vector v (0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1)
 * expanded from seed32, count x 32 bytes to out_host - by the host build of the expander (no GPU) and by its kernel.
 * bh_test_ptau_sums: the eight sums P(V), Q(V) of a transcript as affine records - sums_out[k] (192 bytes each; a G1 record
 * fills the first 96) for k = 2 v + (0 for P, 1 for Q), rcs_out[k] the code of that multiexp; exactly the function
 * bh_powers_of_tau_verify calls. */
void bh_test_ptau_rlc_host(const void *seed32, uint32_t v, size_t count, void *out_host);
int bh_test_ptau_rlc_dev(bh_ctx *ctx, const void *seed32, uint32_t v, size_t count, void *out_host);
int bh_test_ptau_sums(bh_ctx *ctx, const bh_powers_of_tau *t, const void *seed32, void *sums_out, int *rcs_out);

/* ---- the ceremony-step check (csrc/phase2_sums.cuh, csrc/bases_compare.cuh, compiled into this library by
 * csrc/test_phase2_hooks.hip) ---------------------------------------------------------------------------------------
 * bh_test_phase2_sums: the four sums of bh_groth16_params_verify_step as affine G1 records (96 bytes each) - sum rho_i h_i,
 * sum rho_i h'_i (tag 4), sum rho_i l_i, sum rho_i l'_i (tag 5; x' = the element of `after`) - and rcs_out[k] the code of
 * that multiexp; exactly the function the product calls.  An empty query has empty sums: identity records, BH_OK.
 * bh_test_records_differ_host: out[i] = 1 when record i of a differs from record i of b (n dense records of `group`, host
 * arrays, 16-byte aligned), by the host build of the comparison kernel's per-record predicate (no GPU).
 * bh_test_compare_shape: out2 = threads per block, most blocks of one launch of the comparison kernel (a longer range is
 * walked by the same grid in strides). */
int bh_test_phase2_sums(bh_ctx *ctx, const bh_params *before, const bh_params *after, const void *seed32, void *sums_out,
                        int *rcs_out);
int bh_test_records_differ_host(int group, const void *a, const void *b, size_t n, unsigned char *out);
void bh_test_compare_shape(uint32_t out2[2]);

/* ---- the split-scalar point multiplier (csrc/glv.cuh, compiled into this library by csrc/test_point_mul_hooks.hip) ------
 * bh_test_glv_split_host: k1[i] = k[i] mod lambda, k2[i] = k[i] div lambda for n canonical scalars k[i] < q (32 bytes each,
 * little-endian) by the host build of glv_split; k1, k2 hold n x 16 bytes.
 * bh_test_glv_ladder_host / _dev: out[i] = [k1[i] + k2[i] lambda] points[i] as affine records, for ARBITRARY 128-bit pairs
 * (n x 16 bytes each) - not only canonical splits, so that a test reaches the equal- and opposite-point branches of the
 * mixed addition - by the host build of xyzz_mul_glv and by a kernel of one lane per point.  All arrays on the host. */
void bh_test_glv_split_host(const void *k, void *k1, void *k2, size_t n);
int bh_test_glv_ladder_host(int group, const void *points, const void *k1, const void *k2, size_t n, void *out);
int bh_test_glv_ladder_dev(bh_ctx *ctx, int group, const void *points, const void *k1, const void *k2, size_t n, void *out);

/* host only: where bh_msm_sharded_async cuts the exponents for shards of lens[k] bases (cuts_out[n_shards + 1]), and
 * the size class the workspace pool rounds a request up to */
int bh_test_shard_cuts(const size_t *lens, size_t n_shards, size_t skip, const uint64_t *density_words, size_t n_scalars,
                       size_t *cuts_out);
size_t bh_test_pool_size_class(size_t bytes);
/* create_proof's h block + eight multiexps issued as the reference's call sites would issue them through the Rust shim
 * (shim/patches/bellman-hip.patch), transcribed in C++ (csrc/groth16_callsites.cpp):
 *   mode 1  groth16/src/prover.rs patched: bh_scalars_register x2, bh_msm_async_scalars x8, bh_h_poly_fr_scalars
 *   mode 2  only multiexp.rs / domain.rs (/ hip.rs) patched: the EvaluationDomain's vector resident in HBM between its calls,
 *           Exponent::from deferred, every exponent vector registered once (bh_scalars_register), bh_msm_async_scalars x8
 *   mode 0  the round-4 form of that level: 7 x bh_fft_fr on host vectors, the pointwise passes and the
 *           Fr -> Exponent passes on the host, 8 x bh_msm_async with canonical host scalars
 * arguments as bh_groth16_prove_assignment; ms2 (optional): [issue + waits, total] host milliseconds */
int bh_test_groth16_prove_via_call_sites(bh_params *params, int mode, const void *a_evals, const void *b_evals,
                                         const void *c_evals, size_t n_constraints, const void *input_assignment,
                                         size_t n_inputs, const void *aux_assignment, size_t n_aux,
                                         const uint64_t *a_aux_density, const uint64_t *b_input_density,
                                         const uint64_t *b_aux_density, const void *r, const void *s, void *proof_out,
                                         float *ms2);
/* bh_test_many_stage_dev: msm_run_stages once, on the context's stream, under the many-plan make_many_plan gives for k
 * vectors of nd scalars (table != 0: the table flavour over a window table of c bits and `stride` bases per row; else the
 * classic flavour with window size c, stride = 0): the density prefix, msm_many_digits_kernel, the 8-bit sort of every
 * bucket set and the zero-digit search.  scalars: k * nd * 32 bytes, vector v at v * nd * 32 (Montgomery ones below q);
 * density_words optional, ceil(nd / 64) words.  At most 2^22 entries.  Buffers as msm_enqueue sizes them, without its
 * rounding to 256 bytes, each with a guard behind it; ErrFlags starts zeroed, everything else holds the sentinel byte.
 * sorted_out: the W * n sorted pairs (bucket set s at s * n); zstart_out: W words; err_out: one ErrFlags; plan_out4 =
 * [W, entries per set, sort passes, digit columns]; guards_out8: 1 = intact, for pairs_a, pairs_b, counts, scan scratch,
 * zstart, word prefix, ErrFlags, scalars. */
int bh_test_many_stage_dev(bh_ctx *ctx, int table, unsigned c, const void *scalars, int fmt, size_t nd, size_t k,
                           const uint64_t *density_words, size_t skip, size_t n_bases, size_t stride, uint64_t *sorted_out,
                           uint32_t *zstart_out, void *err_out, uint32_t plan_out4[4], uint32_t guards_out8[8]);
/* bh_groth16_prove_witness_batch through its grouped path - five many-jobs per group of witnesses, which the product call
 * does not take by itself (include/bellman_hip.h) - with a workspace budget in bytes of the caller's choice (0: 1 GiB): the
 * witnesses are proved in groups of g with (g + 3) * m * 32 <= workspace_budget, at least one per group; timings4
 * (optional) as the product call, [1] = host time from the start of each group to the issue of its last many-job */
int bh_test_groth16_prove_witness_batch_budget(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                               const void *aux, size_t n_aux, size_t k, const void *r, const void *s,
                                               void *proofs_out, int32_t *rcs, size_t workspace_budget, float *timings4);
/* the same with the path of the caller's choice: mode 0 what the product call does, 1 the grouped path above, 2 the grouped
 * path with a BATCHED h block (groth16.hpp BATCH_GROUPED_H: a, b, c strided per witness, one bh_h_poly_fr_many_dev_on per
 * group; groups of the largest g with 4 * g * m * 32 <= workspace_budget, at least one) */
int bh_test_groth16_prove_witness_batch_mode(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                             const void *aux, size_t n_aux, size_t k, const void *r, const void *s,
                                             void *proofs_out, int32_t *rcs, size_t workspace_budget, int mode, float *timings4);
/* groth16.hpp BATCH_GROUPED_HE (= 3): mode 2 above with the group's constraint evaluations as ONE bh_r1cs_eval_many_dev and,
 * where witness j + 1 starts where witness j ends, one upload per vector kind per group.  An entry point of its own: the
 * hook above keeps refusing every mode beyond 2, as its tests pin. */
int bh_test_groth16_prove_witness_batch_he(bh_params *params, const bh_r1cs *r1cs, const void *inputs, size_t n_inputs,
                                           const void *aux, size_t n_aux, size_t k, const void *r, const void *s,
                                           void *proofs_out, int32_t *rcs, size_t workspace_budget, float *timings4);
/* host only, no GPU: the launches bh_fft_fr_many_dev_on issues with BH_FFT_MANY_FORCE for k vectors of 2^log_n,
 * stride_elems apart, a scratch of scratch_vectors vectors and tables of table_kind (0 two-level, 1 one-level; sizes outside
 * 2^12 .. 2^24 have no one-level tables and plan as 0).  Returns the number of launches (BH_ERR_INVALID_ARG < 0 for a shape
 * the call refuses) and writes the first `cap` of them to out, 20 words each:
 *   [0] grid  [1] threads  [2] one-level kernel  [3] first vector  [4] vectors  [5] reads the scratch  [6] writes the scratch
 *   [7] in stride  [8] out stride (elements; the scratch holds vector [3] + j at j << log_n)
 *   [9] log_n  [10] s  [11] r  [12] log_c  [13] is_last  [14] r0  [15] L  [16] r1  [17] xcd_swizzle   (the pass geometry)
 *   [18] log_v (single-pass sizes: 2^log_v vectors per tile, one per column)  [19] pass */
int bh_test_fft_many_plan(uint32_t log_n, size_t k, size_t stride_elems, size_t scratch_vectors, int table_kind, uint64_t *out,
                          size_t cap);
/* host only, no GPU: the rules of the per-size FFT table cache (csrc/fft_tables_plan.hpp) on plain integers.  What a size
 * holds is (kind, roles, bytes): kind 0 none / 1 one-level / 2 two-level tables; roles bit 0 forward twiddles, 1 inverse
 * twiddles, 2 coset, 3 inverse coset; bytes with the size's 48-byte 1/n entry (0: not cached).
 *   rule 0, what a call does: in[11] = kind, roles, bytes, log_n (< 32), dir (0 forward, 1 inverse), need_tw, need_coset,
 *     need_icoset, bytes the whole cache holds, budget, the BELLMAN_HIP_FFT_ONE_LEVEL switch;  out[4] = bytes of other sizes
 *     to evict first (0: none, then:), the kind to build in, the roles to build, the bytes that adds
 *   rule 1, after a failed one-level build: in[4] = kind, roles, bytes, bytes the other sizes hold;  out[1] = 0 fall back to
 *     two-level tables, 1 evict every other size and retry, 2 fail
 *   rule 2, the next size an eviction drops: in[4 + 3 * sizes] = the size to keep, bytes the cache holds, bytes to make room
 *     for (UINT64_MAX: drop everything else), budget, then (log_n, bytes, last use) per size;  out[1] = its index, UINT64_MAX: none
 * Returns BH_OK, or BH_ERR_INVALID_ARG for another rule, another n_in or log_n >= 32. */
int bh_test_fft_table_policy(int rule, const uint64_t *in, size_t n_in, uint64_t *out);
/* host only: the number of witnesses a lane of bh_r1cs_eval_many_dev / bh_r1cs_check_many_dev serves (csrc/r1cs_dev.hpp
 * R1CS_MANY_TILE), so that a test can place k on the tile edges */
uint32_t bh_test_r1cs_many_tile(void);
/* host only: the witness solver's planner (csrc/solve_plan.hpp) on the caller's CSR arrays, no context: abc / coeffs as
 * bh_r1cs_create takes them, desc as bh_r1cs_solver_create.  Returns the planner's status (BH_OK / BH_ERR_INVALID_ARG) with
 * *first_unsolved as bh_r1cs_solver_create reports it.  With BH_OK, per variable: definer[v] = -1 (ONE, supplied), the
 * defining constraint i >= 0, or -2 - h for an output of hint h; level[v]; counts5 as bh_r1cs_solver_info. */
int bh_test_r1cs_solve_plan(size_t n_inputs, size_t n_aux, size_t n_constraints, const bh_csr abc[3], const void *coeffs,
                            size_t n_coeffs, const bh_solver_desc *desc, uint32_t *first_unsolved, int64_t *definer,
                            uint32_t *level, size_t counts5[5]);
/* the launch forms of bh_r1cs_solve_many_dev for the calls that follow on this solver (csrc/r1cs_dev.hpp): form 0 = chosen
 * per level, 1 = every level in the walk kernel, 2 = one launch per level; witnesses_per_group 0 = chosen per run;
 * level_min_items 0 = the shipped switch point.  Not thread-safe: between calls only. */
int bh_test_r1cs_solver_tune(bh_r1cs_solver *s, uint32_t form, uint32_t witnesses_per_group, uint64_t level_min_items);
/* bh_groth16_prove_witness_batch_dev with a path of its own (groth16.hpp): mode 0 the call as shipped, mode 3
 * BATCH_GROUPED_HE - five many-jobs, one bh_r1cs_eval_many_dev and one batched h block per group, a group being a run of
 * consecutive proved witnesses (under BH_PROVE_CHECK an unsatisfied witness ends it) with 4 * g * m * 32 <= workspace_budget
 * (0: the default), read through the caller's pointers and strides.  Any other mode is BH_ERR_INVALID_ARG. */
int bh_test_groth16_prove_witness_batch_dev_mode(bh_params *params, const bh_r1cs *r1cs, const void *inputs_dev, size_t in_stride,
                                                 const void *aux_dev, size_t aux_stride, size_t k, const void *r, const void *s,
                                                 unsigned flags, void *stream, void *proofs_out, int32_t *rcs,
                                                 uint32_t *first_unsatisfied, float *timings4, size_t workspace_budget, int mode);
/* host only, no GPU: bh_groth16_assemble_many's arguments and results, computed by the HOST compilation of the device
 * functions of csrc/proof_finish.cuh - the text the kernels compile, lane by lane */
int bh_test_proof_finish_host(bh_params *params, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                              int32_t *rcs);
/* the same with the verifying key's five points handed over as bh_proof_finish_dev takes them (vk5, BH_FINISH_KEY_BYTES):
 * needs no bh_params, which only exist with a device context */
int bh_test_proof_finish_host_vk(const void *vk5, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                                 int32_t *rcs);
/* host only, no context: the word-program validator and interpreter (csrc/word_program.hpp) on a descriptor as
 * bh_word_witness_create takes it.  Returns BH_OK, or BH_ERR_INVALID_ARG with bad_index as bh_word_witness_create reports it.
 * With BH_OK and ext (n_ext uint32) not NULL, one witness is interpreted on the host: inputs_out [n_inputs] and aux_out
 * [n_aux] Montgomery Fr, words_out (may be NULL) the n_ext + n_instrs trace words. */
int bh_test_word_program(const bh_word_witness_desc *desc, uint32_t bad_index[2], const uint32_t *ext, void *inputs_out,
                         void *aux_out, uint64_t *words_out);
/* witnesses per scratch chunk of bh_word_witness_generate_dev for the calls that follow on this handle (0: the shipped
 * bound, csrc/r1cs_dev.hpp WORD_SCRATCH_MAX_BYTES).  Not thread-safe: between calls only. */
int bh_test_word_witness_chunk(bh_word_witness *w, size_t witnesses_per_chunk);

#ifdef __cplusplus
}
#endif
#endif
