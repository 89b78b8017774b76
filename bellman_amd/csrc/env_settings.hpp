// Every environment variable the library reads, in one place (INTEGRATION.md section 4 documents them).  Host-only, plain C++:
// the .hip units and the host objects of libbellman_groth16.a both include it.  The BELLMAN_HIP_* variables and BH_DEBUG are
// read once, at the first call of env(); a plan is never shaped by a variable that is not listed here.
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace bh {

struct EnvSettings {
  static constexpr size_t UNSET = (size_t)-1;   // (a byte count parsed from megabytes has its low 20 bits clear)
  int table_max_log2 = -1;        // BELLMAN_HIP_TABLE_MAX_LOG2: largest vector that gets an automatic window table, both groups
  int table_max_log2_g1 = -1;     // BELLMAN_HIP_TABLE_MAX_LOG2_G1: the G1 limit alone (both: clamped to 0 ... 24, 0 = never, -1 = unset)
  bool table_pad = true;          // BELLMAN_HIP_TABLE_PAD=0: G1 tables of 2^19 points and more stay dense (tests/test_gpu_round4.py test_g1_window_table_at_128_byte_stride)
  bool fft_one_level = true;      // BELLMAN_HIP_FFT_ONE_LEVEL=0: hi x lo twiddle tables at every size (tests)
  long max_jobs = 0;              // BELLMAN_HIP_MAX_JOBS: jobs in flight per context (<= 0: from the device's memory)
  size_t table_budget = UNSET;    // BELLMAN_HIP_TABLE_BUDGET_MB, in bytes
  size_t fft_table_budget = UNSET;   // BELLMAN_HIP_FFT_TABLE_BUDGET_MB, in bytes
  size_t pool_cap = UNSET;        // BELLMAN_HIP_POOL_CAP_MB, in bytes
  bool verify_each_shared = false;   // BELLMAN_HIP_VERIFY_EACH_SHARED=1: one three-pair Miller loop per proof, shared squarings (tools/bench_verify_each.py)
  bool debug = false;             // BH_DEBUG (set to anything): the prover's trace on stderr
};

inline const EnvSettings &env() {
  static const EnvSettings s = [] {
    EnvSettings v;
    auto text = [](const char *name) { const char *e = getenv(name); return e && *e ? e : nullptr; };
    auto log2_limit = [&](const char *name) {
      const char *e = text(name);
      if (!e) return -1;
      const long x = strtol(e, nullptr, 10);
      return (int)(x < 0 ? 0 : x > 24 ? 24 : x);
    };
    auto not_zero = [](const char *name) { const char *e = getenv(name); return !(e && *e == '0'); };
    auto megabytes = [&](const char *name) {
      const char *e = text(name);
      return e ? (size_t)strtoull(e, nullptr, 10) << 20 : EnvSettings::UNSET;
    };
    v.table_max_log2 = log2_limit("BELLMAN_HIP_TABLE_MAX_LOG2");
    v.table_max_log2_g1 = log2_limit("BELLMAN_HIP_TABLE_MAX_LOG2_G1");
    v.table_pad = not_zero("BELLMAN_HIP_TABLE_PAD");
    v.fft_one_level = not_zero("BELLMAN_HIP_FFT_ONE_LEVEL");
    if (const char *e = text("BELLMAN_HIP_MAX_JOBS")) v.max_jobs = strtol(e, nullptr, 10);
    v.table_budget = megabytes("BELLMAN_HIP_TABLE_BUDGET_MB");
    v.fft_table_budget = megabytes("BELLMAN_HIP_FFT_TABLE_BUDGET_MB");
    v.pool_cap = megabytes("BELLMAN_HIP_POOL_CAP_MB");
    if (const char *e = text("BELLMAN_HIP_VERIFY_EACH_SHARED")) v.verify_each_shared = *e != '0';
    v.debug = getenv("BH_DEBUG") != nullptr;
    return v;
  }();
  return s;
}

// GPU_MAX_HW_QUEUES belongs to the HIP runtime, and bh_runtime_configure may set it: read afresh at every call, never cached
inline int env_hw_queues() {
  const char *q = getenv("GPU_MAX_HW_QUEUES");
  return (q && *q) ? atoi(q) : 0;
}

}  // namespace bh
