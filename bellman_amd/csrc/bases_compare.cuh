// Comparison of resident point records (bh_bases_first_difference, api_bases.hip): the first index at which two ranges of dense
// 96- / 192-byte records differ.  One lane per record; a record is read as VEC 16-byte vectors (6 for G1, 12 for G2) and
// the two sides are XORed into one word, so a lane holds two vectors and an accumulator at a time - no scratch, few
// registers, full occupancy.  The wavefront's lanes are combined by a ballot; one 64-bit atomicMin per wavefront that saw
// a difference.  The kernel does no arithmetic to speak of: it is bound by the 2 x count x 96|192 bytes it reads.
// Included by api_bases.hip (the product) and by test_phase2_hooks.hip (the test library), which runs the predicate on the host.
#pragma once
#include "common.hpp"

namespace bh {

static constexpr u32 COMPARE_THREADS = 256;
// 8 blocks of 4 wavefronts per CU on 256 CUs: the grid that fills the chip once; longer ranges stride over it
static constexpr u32 COMPARE_MAX_BLOCKS = 2048;

// the per-record predicate: do the VEC 16-byte vectors at a and b differ anywhere?
template <int VEC>
BH_HD bool records_differ(const uint4 *a, const uint4 *b) {
  u32 d = 0;
#pragma unroll 2
  for (int k = 0; k < VEC; k++) {
    const uint4 x = a[k], y = b[k];
    d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
  }
  return d != 0;
}

// *min_idx (preset to ~0) <- the smallest i < count with record i of a != record i of b
template <int VEC>
__global__ __launch_bounds__(COMPARE_THREADS) void first_difference_kernel(const uint4 *a, const uint4 *b, u64 count,
                                                                            unsigned long long *min_idx) {
  // (the loop bound is the same for every lane of a block, so every ballot is taken by whole wavefronts)
  for (u64 base = (u64)blockIdx.x * COMPARE_THREADS; base < count; base += (u64)gridDim.x * COMPARE_THREADS) {
    const u64 i = base + threadIdx.x;
    const bool differ = i < count && records_differ<VEC>(a + i * VEC, b + i * VEC);
    const u64 ballot = __ballot(differ);
    if (ballot && (threadIdx.x & 63) == 0) atomicMin(min_idx, (unsigned long long)(i + (u64)(__ffsll((long long)ballot) - 1)));
  }
}

static inline int launch_first_difference(hipStream_t st, int group, const void *a, const void *b, u64 count,
                                          unsigned long long *min_idx) {
  if (!count) return BH_OK;
  const u64 blocks = (count + COMPARE_THREADS - 1) / COMPARE_THREADS;
  const dim3 grid((u32)(blocks < COMPARE_MAX_BLOCKS ? blocks : COMPARE_MAX_BLOCKS));
  (void)hipGetLastError();
  if (group == BH_G1)
    hipLaunchKernelGGL(first_difference_kernel<6>, grid, dim3(COMPARE_THREADS), 0, st, (const uint4 *)a, (const uint4 *)b, count, min_idx);
  else
    hipLaunchKernelGGL(first_difference_kernel<12>, grid, dim3(COMPARE_THREADS), 0, st, (const uint4 *)a, (const uint4 *)b, count, min_idx);
  BH_HIP_CHECK(hipGetLastError());
  return BH_OK;
}

}  // namespace bh
