// Host-only policy of the per-size FFT table cache (fft.hip get_tables / fft_evict_locked): which kind of tables a domain
// size runs on, what a call has to build and what that costs against the cache's budget, what follows a failed one-level
// build, and which size an eviction drops next.  Plain values in, plain values out - no HIP call, no Context, no lock: the
// test library replays these rules without a GPU (bh_test_fft_table_policy, tests/test_fft_table_cache_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bh {

// One kind of tables per size: the one-level kernel multiplies by whatever its table pointers say, and the 1/n sits in a
// different table in either kind (fft.hip FFT_ROLE_SPECS), so the two kinds are never mixed within a size.  A size counts as
// running on a kind only once it HOLDS a table of it: a call that built none - a cached 1/Z, a single-pass request - leaves
// NONE and must not let later calls skip the budget gate of fft_tables_decide.  Evicting a size forgets its kind.
enum FftTableKind : uint32_t { FFT_TABLES_NONE = 0, FFT_TABLES_ONE_LEVEL = 1, FFT_TABLES_TWO_LEVEL = 2 };
// what a table is for; a size holds each role or not (bit 1 << role of a role mask)
enum FftTableRole : uint32_t { FFT_ROLE_TW_FWD = 0, FFT_ROLE_TW_INV = 1, FFT_ROLE_COSET = 2, FFT_ROLE_ICOSET = 3, FFT_ROLES = 4 };

constexpr size_t FFT_ONE_LEVEL_ENTRY_BYTES = 32;   // the Montgomery element (fft.hip NTT_ONE_STRIDE)
constexpr size_t FFT_TWO_LEVEL_ENTRY_BYTES = 48;   // B form (common.hpp BTw)
constexpr size_t FFT_MINV_BYTES = FFT_TWO_LEVEL_ENTRY_BYTES;   // the one-entry 1/n table every cached size holds
constexpr size_t FFT_EVICT_ALL = (size_t)-1;

// what a size holds: bytes counts its tables and its 1/n entry (0: the size is not cached), not the shared master tables
struct FftHoldings {
  uint32_t kind = FFT_TABLES_NONE, roles = 0;
  size_t bytes = 0;
};

// dir: 0 forward, 1 inverse
inline uint32_t fft_roles_needed(int dir, bool need_tw, bool need_coset, bool need_icoset) {
  return (need_tw ? 1u << (FFT_ROLE_TW_FWD + dir) : 0) | (need_coset ? 1u << FFT_ROLE_COSET : 0) | (need_icoset ? 1u << FFT_ROLE_ICOSET : 0);
}
// a one-level table has n entries; a twiddle role is one table per non-last pass, a coset role one table
inline size_t fft_one_level_role_bytes(uint32_t role, uint32_t log_n, uint32_t passes) {
  return (role <= FFT_ROLE_TW_INV ? (size_t)(passes - 1) : (size_t)1) * (FFT_ONE_LEVEL_ENTRY_BYTES << log_n);
}
// the complete one-level set of a size: an inter-pass twiddle table per non-last pass and direction, 7^i, 7^-i
inline size_t fft_one_level_set_bytes(uint32_t log_n, uint32_t passes) {
  size_t b = 0;
  for (uint32_t role = 0; role < FFT_ROLES; role++) b += fft_one_level_role_bytes(role, log_n, passes);
  return b;
}
// two-level tables: entry e of a virtual n-entry table is hi[e >> lb] * lo[e & (2^lb - 1)]; a role is one lo / hi pair
inline uint32_t fft_two_level_low_bits(uint32_t log_n) { return (log_n + 1) / 2; }
inline size_t fft_two_level_role_bytes(uint32_t log_n) {
  const uint32_t lb = fft_two_level_low_bits(log_n);
  return (((size_t)1 << lb) + ((size_t)1 << (log_n - lb))) * FFT_TWO_LEVEL_ENTRY_BYTES;
}
// the device memory `roles` take in `kind`, beside the 1/n entry of a size that is not cached yet
inline size_t fft_tables_build_bytes(const FftHoldings &h, uint32_t kind, uint32_t roles, uint32_t log_n, uint32_t passes) {
  size_t b = h.bytes ? 0 : FFT_MINV_BYTES;
  for (uint32_t role = 0; role < FFT_ROLES; role++)
    if (roles >> role & 1) b += kind == FFT_TABLES_ONE_LEVEL ? fft_one_level_role_bytes(role, log_n, passes) : fft_two_level_role_bytes(log_n);
  return b;
}

// evict_need != 0: that many bytes of OTHER sizes' tables have to go first (fft_evict_victim), then decide again.
// Otherwise: build `roles` (possibly none) in `kind`, which adds `bytes` to the size and to the cache.
struct FftTableDecision {
  size_t evict_need = 0;
  uint32_t kind = FFT_TABLES_NONE, roles = 0;
  size_t bytes = 0;
};
// What a call that needs the roles of (dir, need_*) at a size of `passes` passes does, `h` being what the size holds,
// cache_bytes what all sizes hold and one_level_enabled the BELLMAN_HIP_FFT_ONE_LEVEL switch.
// One-level tables (n entries each: 0.13 GB at 2^22, 0.5 GB at 2^24) where the size's COMPLETE set fits the cache's
// budget - so that dropping the other sizes always makes room for whichever of its tables is asked for next, and the
// kind of tables a size uses never changes while it is cached.  A size that holds two-level tables (over budget, a failed
// allocation) keeps them.
inline FftTableDecision fft_tables_decide(const FftHoldings &h, uint32_t log_n, uint32_t passes, int dir, bool need_tw, bool need_coset,
                                          bool need_icoset, size_t cache_bytes, size_t budget, bool one_level_enabled) {
  FftTableDecision d;
  d.kind = h.kind;
  if (d.kind == FFT_TABLES_NONE)
    d.kind = one_level_enabled && log_n >= 12 && log_n <= 24 && fft_one_level_set_bytes(log_n, passes) <= budget ? FFT_TABLES_ONE_LEVEL
                                                                                                                  : FFT_TABLES_TWO_LEVEL;
  d.roles = fft_roles_needed(dir, need_tw, need_coset, need_icoset) & ~h.roles;
  if (d.kind == FFT_TABLES_ONE_LEVEL) {
    size_t need = 0;
    for (uint32_t role = 0; role < FFT_ROLES; role++)
      if (d.roles >> role & 1) need += fft_one_level_role_bytes(role, log_n, passes);
    if (need && cache_bytes + need > budget) {
      if (cache_bytes > h.bytes) { d.evict_need = need; return d; }   // other sizes to drop (nothing built yet: nothing to undo)
      if (h.kind != FFT_TABLES_ONE_LEVEL) d.kind = FFT_TABLES_TWO_LEVEL;   // the budget was lowered under this call: two-level tables
      // (a size that already runs on one-level tables completes its set: at most its own set over the new budget)
    }
  }
  d.bytes = fft_tables_build_bytes(h, d.kind, d.roles, log_n, passes);
  return d;
}

// What follows a ONE-LEVEL build of which an allocation or a launch failed (a failed two-level build has nothing to fall
// back to: the call fails).  other_bytes: what the other sizes hold.
//   FALL_BACK_TWO_LEVEL  drop this call's fresh one-level tables and build its roles two-level: the size stays on the
//                        two-level tables for good
//   EVICT_ALL_AND_RETRY  drop this call's fresh tables and every other size (FFT_EVICT_ALL), then decide again
//   FAIL                 the call fails
// A size that already runs on one-level tables (its inverse twiddles carry the 1/n) must not fall back to the two-level
// kind half way (a forward call whose allocation failed after an inverse call had built its tables ran the
// one-level kernel with null table pointers) - it makes room by dropping the other sizes, and if there is nothing to drop
// the call fails.  A size without tables yet also tries that before it gives up.
enum FftBuildFailure : uint32_t { FFT_FALL_BACK_TWO_LEVEL = 0, FFT_EVICT_ALL_AND_RETRY = 1, FFT_FAIL = 2 };
inline FftBuildFailure fft_tables_build_failed(const FftHoldings &h, size_t other_bytes) {
  if (other_bytes) return FFT_EVICT_ALL_AND_RETRY;
  return h.kind == FFT_TABLES_ONE_LEVEL ? FFT_FAIL : FFT_FALL_BACK_TWO_LEVEL;
}

// The next size an eviction drops: the least recently used one other than `keep_log_n` that holds anything, until `need`
// more bytes fit the budget beside cache_bytes (FFT_EVICT_ALL: until nothing else is left).  Returns its index, -1: done.
struct FftCacheEntry {
  uint32_t log_n;
  size_t bytes;
  uint64_t last_use;
};
inline int fft_evict_victim(const FftCacheEntry *e, size_t count, uint32_t keep_log_n, size_t cache_bytes, size_t need, size_t budget) {
  if (need != FFT_EVICT_ALL && cache_bytes + need <= budget) return -1;
  int victim = -1;
  for (size_t i = 0; i < count; i++)
    if (e[i].log_n != keep_log_n && e[i].bytes && (victim < 0 || e[i].last_use < e[victim].last_use)) victim = (int)i;
  return victim;
}

}  // namespace bh
