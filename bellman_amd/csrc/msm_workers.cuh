// Logical workers of the MSM kernels: how a thread finds the worker it belongs to, in every lane form of the field bundles.
#pragma once
#include "fp2pair.cuh"

namespace bh {

// ---------------------------------------------------------------------------------------------------------
// Logical workers.  A kernel below is written for "workers": one thread when a lane holds a whole group
// element (F::LANES == 1: G1, single-lane G2), one lane TRIPLE for the K3 form of G2 (fp2k3.cuh), where a
// wavefront carries PER_WAVE triples - 21, or 16 where shuffle trees want a power of two - or one lane PAIR
// (fp2pair.cuh, 32 per wavefront).  All lanes of a worker see the same worker index and take the same branches
// (every predicate of the curve code is uniform over the worker's lanes).
// ---------------------------------------------------------------------------------------------------------
template <class F>
constexpr u32 default_per_wave() { return F::LANES == 3 ? 21u : F::LANES == 2 ? 32u : 64u; }
template <class F>
constexpr u32 tree_per_wave() { return F::LANES == 3 ? 16u : F::LANES == 2 ? 32u : 64u; }
template <class F>
constexpr u32 workers_per_block(u32 threads, u32 per_wave) { return F::LANES == 1 ? threads : (threads / 64u) * per_wave; }

// which of its worker's lanes a thread is (0 = the lane that speaks for the worker)
template <class F>
__device__ __forceinline__ u32 worker_role() {
  if constexpr (F::LANES == 1) return 0u;
  else if constexpr (F::LANES == 2) return pair_role();
  else return k3_role();
}
// false for lanes that carry no worker (lane 63 of a K3 wavefront, lanes beyond PER_WAVE triples)
template <class F>
__device__ __forceinline__ bool worker_index(u32 per_wave, u32 &in_block, u32 &global) {
  if constexpr (F::LANES == 1) {
    in_block = threadIdx.x;
    global = blockIdx.x * blockDim.x + threadIdx.x;
    return true;
  } else {
    const u32 t = F::LANES == 3 ? k3_triple(threadIdx.x & 63u) : (threadIdx.x & 63u) >> 1;
    const u32 wave = threadIdx.x >> 6, waves_per_block = blockDim.x >> 6;
    in_block = wave * per_wave + t;
    global = (blockIdx.x * waves_per_block + wave) * per_wave + t;
    return t < per_wave;
  }
}

}  // namespace bh
