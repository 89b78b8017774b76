// Witnesses of a gadget circuit from its word program: k witnesses computed ON the device from their external words (for a
// SHA-256 preimage circuit, the message) - what the value closures of `synthesize` compute on one host thread, one variable
// at a time, while the circuit is walked (groth16/src/prover.rs:206 for circuits built from src/gadgets/uint32.rs).  The
// program format, its validator and the one definition of what an instruction computes are word_program.hpp (host only);
// this file holds the two kernels and the C ABI.
//
//   RUN      one lane per witness walks the whole program: the instruction records are the same for every lane (uniform,
//            read-only loads), the lanes differ only in the witness they serve.  Word w of witness j lives at
//            words[w * stride + j], so the 64 lanes of a wavefront read and write 64 consecutive u64 - whole lines.  A lane
//            re-reads only what it wrote itself: no ordering between lanes, wavefronts or workgroups is needed, and there
//            are no flags and no barriers.  The word-file pointer carries neither const nor __restrict__: no load of it
//            may be routed through a read-only path or hoisted over the store it follows (as r1cs_solve.hip).
//   EXPAND   a launch of its own behind it (the launch boundary is the ordering): consecutive lanes write consecutive
//            variables of one witness, 32 bytes each - Montgomery 0 or R for a bit, the canonical sum times R^2 (one
//            ff.cuh product) for a packed variable, R for ONE - so a wavefront stores 2 KiB of whole lines.  Lanes whose
//            variables are bits of one word (the 32 results of a UInt32 operation are allocated in a row) read the same u64.
//            Bytes between n * 32 and the stride are never written.
// The two are not fused: RUN has k lanes of work, EXPAND k * n_vars; a fused kernel would write a witness's 0.8 MB from one
// lane in 32-byte pieces a whole stride apart.
#include <string.h>

#include <algorithm>
#include <vector>

#include "r1cs_dev.hpp"

using namespace bh;

namespace {

struct WordArgs {
  const uint4 *instrs;
  const u32 *pool;
  const uint2 *bits;
  const uint2 *recs;
  u64 *words;               // written AND re-read by RUN; read by EXPAND
  const char *ext;          // witness j's external words (u32) at ext + j * ext_stride
  char *inputs, *aux;       // witness j at inputs + j * in_stride, aux + j * aux_stride
  u64 ext_stride, in_stride, aux_stride;
  u64 k;                    // witnesses of this launch
  u64 stride;               // of the word file, in words: >= k
  u32 n_ext, n_instrs, n_inputs, n_vars;
};

__global__ void __launch_bounds__(WORD_RUN_LANES) word_run_kernel(WordArgs a) {
  const u64 j = (u64)blockIdx.x * WORD_RUN_LANES + threadIdx.x;
  if (j >= a.k) return;
  u64 *wf = a.words + j;
  const u64 stride = a.stride;
  const u32 *ext = reinterpret_cast<const u32 *>(a.ext + j * a.ext_stride);
  for (u32 e = 0; e < a.n_ext; e++) wf[(u64)e * stride] = ext[e];
  auto load = [&](u32 w) -> u64 { return wf[(u64)w * stride]; };
  const WordBit *bits = reinterpret_cast<const WordBit *>(a.bits);
  for (u32 i = 0; i < a.n_instrs; i++) {
    const uint4 q = a.instrs[i];
    const WordInstr in = {q.x, q.y, q.z, q.w};
    wf[(u64)(a.n_ext + i) * stride] = word_exec(in, a.pool, bits, load);
  }
}

// the canonical integer of a packed variable, limb by limb (no dynamic index into the limbs: they stay in registers)
__device__ __attribute__((noinline)) fr_t word_packed_value(const uint2 *bits, u32 begin, u32 n_bits, const u64 *wf, u64 stride) {
  fr_t c;
#pragma unroll
  for (u32 l = 0; l < 8; l++) {
    u32 limb = 0;
    for (u32 b = 0; b < 32 && l * 32 + b < n_bits; b++) {
      const uint2 s = bits[begin + l * 32 + b];
      limb |= (u32)(((wf[(u64)s.x * stride] >> (s.y & 63)) ^ (s.y >> 8)) & 1) << b;
    }
    c.l[l] = limb;
  }
  fr_t r;
  fe_to_mont(r, c);
  return r;
}

__global__ void __launch_bounds__(WORD_EXPAND_LANES) word_expand_kernel(WordArgs a) {
  const u32 v = blockIdx.x * WORD_EXPAND_LANES + threadIdx.x;
  if (v >= a.n_vars) return;
  const uint2 rec = a.recs[v];
  const u32 kind = (rec.y >> 16) & 3;
  fr_t one, zero;
  fe_one(one);
  fe_zero(zero);
  for (u64 j = blockIdx.y; j < a.k; j += gridDim.y) {
    const u64 *wf = a.words + j;
    fr_t out = one;
    if (kind == WORD_REC_BIT) {
      out = (((wf[(u64)rec.x * a.stride] >> (rec.y & 63)) ^ (rec.y >> 8)) & 1) ? one : zero;
    } else if (kind == WORD_REC_PACKED) {
      out = word_packed_value(a.bits, rec.x, rec.y & 0xFFFF, wf, a.stride);
    }
    fr_t *dst = v < a.n_inputs ? reinterpret_cast<fr_t *>(a.inputs + j * a.in_stride) + v
                               : reinterpret_cast<fr_t *>(a.aux + j * a.aux_stride) + (v - a.n_inputs);
    st_fr16(dst, out);
  }
}

constexpr u32 EXPAND_MAX_ROWS = 65535;   // gridDim.y

}  // namespace

extern "C" {

int bh_word_witness_create(bh_ctx *ctx, const bh_word_witness_desc *desc, bh_word_witness **out, uint32_t bad_index[2]) {
  if (bad_index) { bad_index[0] = 0; bad_index[1] = WORD_NO_INDEX; }
  if (!ctx || !desc || !out) return BH_ERR_INVALID_ARG;
  static_assert(sizeof(bh_word_instr) == sizeof(WordInstr) && sizeof(bh_word_bit) == sizeof(WordBit) && sizeof(bh_word_var) == sizeof(WordVar) &&
                    sizeof(bh_word_packed) == sizeof(WordPacked) && sizeof(bh_word_witness_desc) == sizeof(WordDesc) &&
                    sizeof(WordInstr) == sizeof(uint4) && sizeof(WordBit) == sizeof(uint2) && sizeof(WordRec) == sizeof(uint2),
                "record layouts");
  const WordDesc &d = *reinterpret_cast<const WordDesc *>(desc);
  const WordProgram p = word_program_validate(d);
  if (p.status != WORD_OK) {
    if (bad_index) { bad_index[0] = p.bad_code; bad_index[1] = p.bad_index; }
    return BH_ERR_INVALID_ARG;
  }
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  bh_word_witness *w = new bh_word_witness;
  w->ctx = ctx;
  w->n_inputs = d.n_inputs; w->n_aux = d.n_aux; w->n_ext = d.n_ext; w->n_instrs = d.n_instrs; w->n_words = p.n_words;
  int rc = r1cs_upload_vec(ctx, &w->instrs, reinterpret_cast<const uint4 *>(d.instrs), d.n_instrs);
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &w->pool, d.pool, d.n_pool);
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &w->bits, reinterpret_cast<const uint2 *>(d.bits), d.n_bits);
  if (rc == BH_OK) rc = r1cs_upload_vec(ctx, &w->recs, reinterpret_cast<const uint2 *>(p.recs.data()), p.recs.size());
  if (rc == BH_OK && hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess) rc = BH_ERR_HIP;
  if (rc == BH_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = BH_ERR_HIP;   // the sources are the caller's and locals
  if (rc != BH_OK) { bh_word_witness_destroy(w); return rc; }
  *out = w;
  return BH_OK;
}

void bh_word_witness_destroy(bh_word_witness *w) {
  if (!w) return;
  if (w->done) {
    if (w->used) (void)hipEventSynchronize(w->done);   // the last call's kernels read the tables and the scratch
    (void)hipEventDestroy(w->done);
  }
  w->ctx->c.pool.release(w->instrs);
  w->ctx->c.pool.release(w->pool);
  w->ctx->c.pool.release(w->bits);
  w->ctx->c.pool.release(w->recs);
  w->ctx->c.pool.release(w->scratch);
  delete w;
}

int bh_word_witness_generate_dev(bh_ctx *ctx, const bh_word_witness *cw, const void *ext_dev, size_t ext_stride, void *inputs_dev,
                                 size_t in_stride, void *aux_dev, size_t aux_stride, size_t k, void *stream) {
  bh_word_witness *w = const_cast<bh_word_witness *>(cw);   // (the scratch and its ordering are the handle's own business)
  if (!ctx || !w || w->ctx != ctx) return BH_ERR_INVALID_ARG;
  if (in_stride % 32 || aux_stride % 32 || in_stride < w->n_inputs * 32 || aux_stride < w->n_aux * 32 || !inputs_dev ||
      (w->n_aux && !aux_dev) || ext_stride % 4 || ext_stride < w->n_ext * 4 || (w->n_ext && !ext_dev))
    return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->c.stream;
  std::lock_guard<std::mutex> g(w->mu);
  const size_t words = std::max<size_t>(w->n_words, 1);
  size_t chunk = w->force_chunk ? w->force_chunk : std::max<size_t>(WORD_SCRATCH_MAX_BYTES / (words * 8), WORD_RUN_LANES);
  chunk = std::min(chunk, k);
  const size_t stride = (chunk + WORD_RUN_LANES - 1) / WORD_RUN_LANES * WORD_RUN_LANES;   // rows of the word file start on a line
  const size_t need = words * stride * 8;
  if (w->used) BH_HIP_CHECK(hipStreamWaitEvent(st, w->done, 0));   // the previous call may have run on another stream
  if (need > w->scratch_bytes) {
    if (w->used) BH_HIP_CHECK(hipEventSynchronize(w->done));
    ctx->c.pool.release(w->scratch);
    w->scratch_bytes = 0;
    w->scratch = (u64 *)ctx->c.pool.acquire(need);
    if (!w->scratch) return BH_ERR_HIP;
    w->scratch_bytes = need;
  }
  WordArgs a;
  a.instrs = w->instrs; a.pool = w->pool; a.bits = w->bits; a.recs = w->recs;
  a.words = w->scratch;
  a.ext_stride = ext_stride; a.in_stride = in_stride; a.aux_stride = aux_stride;
  a.stride = stride;
  a.n_ext = (u32)w->n_ext; a.n_instrs = (u32)w->n_instrs; a.n_inputs = (u32)w->n_inputs; a.n_vars = (u32)(w->n_inputs + w->n_aux);
  const u32 var_blocks = (a.n_vars + WORD_EXPAND_LANES - 1) / WORD_EXPAND_LANES;
  for (size_t first = 0; first < k; first += chunk) {
    const size_t n = std::min(chunk, k - first);
    a.ext = (const char *)ext_dev + first * ext_stride;
    a.inputs = (char *)inputs_dev + first * in_stride;
    a.aux = (char *)aux_dev + first * aux_stride;
    a.k = n;
    hipLaunchKernelGGL(word_run_kernel, dim3((u32)((n + WORD_RUN_LANES - 1) / WORD_RUN_LANES)), dim3(WORD_RUN_LANES), 0, st, a);
    BH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(word_expand_kernel, dim3(var_blocks, (u32)std::min<size_t>(n, EXPAND_MAX_ROWS)), dim3(WORD_EXPAND_LANES), 0, st, a);
    BH_HIP_CHECK(hipGetLastError());
  }
  BH_HIP_CHECK(hipEventRecord(w->done, st));
  w->used = true;
  return BH_OK;
}

int bh_word_witness_generate(bh_ctx *ctx, const bh_word_witness *w, const void *ext_host, void *inputs_host, void *aux_host, size_t k) {
  if (!ctx || !w || w->ctx != ctx) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!inputs_host || (w->n_aux && !aux_host) || (w->n_ext && !ext_host)) return BH_ERR_INVALID_ARG;
  BH_HIP_CHECK(hipSetDevice(ctx->c.device));
  const size_t in_bytes = w->n_inputs * 32, aux_bytes = w->n_aux * 32, ext_bytes = w->n_ext * 4;
  // groups of witnesses whose device copies stay within 1 GiB, at least one witness per group (as bh_r1cs_solve_many)
  const size_t group = std::min(k, std::max<size_t>((size_t(1) << 30) / (in_bytes + aux_bytes), 1));
  void *stream = nullptr;
  int rc = bh_stream_create(ctx, &stream);   // a stream of its own: thread-safe
  if (rc != BH_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  void *d_in = ctx->c.pool.acquire(group * in_bytes + 32), *d_aux = ctx->c.pool.acquire(group * aux_bytes + 32);
  void *d_ext = ctx->c.pool.acquire(group * ext_bytes + 32);
  if (!d_in || !d_aux || !d_ext) rc = BH_ERR_HIP;
  auto hip_ok = [&](hipError_t e) {
    if (e != hipSuccess) {
      fprintf(stderr, "[bellman_hip] bh_word_witness_generate: %s\n", hipGetErrorString(e));
      rc = BH_ERR_HIP;
    }
    return e == hipSuccess;
  };
  for (size_t first = 0; first < k && rc == BH_OK; first += group) {
    const size_t g = std::min(group, k - first);
    if (ext_bytes && !hip_ok(hipMemcpyAsync(d_ext, (const char *)ext_host + first * ext_bytes, g * ext_bytes, hipMemcpyHostToDevice, st))) break;
    rc = bh_word_witness_generate_dev(ctx, w, d_ext, ext_bytes, d_in, in_bytes, d_aux, aux_bytes, g, stream);
    if (rc != BH_OK) break;
    if (!hip_ok(hipMemcpyAsync((char *)inputs_host + first * in_bytes, d_in, g * in_bytes, hipMemcpyDeviceToHost, st))) break;
    if (aux_bytes && !hip_ok(hipMemcpyAsync((char *)aux_host + first * aux_bytes, d_aux, g * aux_bytes, hipMemcpyDeviceToHost, st))) break;
    if (!hip_ok(hipStreamSynchronize(st))) break;   // the group's buffers are written again by the next one
  }
  (void)hipStreamSynchronize(st);
  ctx->c.pool.release(d_in);
  ctx->c.pool.release(d_aux);
  ctx->c.pool.release(d_ext);
  bh_stream_destroy(ctx, stream);
  return rc;
}

}  // extern "C"
