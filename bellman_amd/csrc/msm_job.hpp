// What msm.hip exports: the life of a multiexp job as the C API drives it (api_msm.hip; the context's back-pressure and
// bookkeeping in api_context.hip), and the fixed-base multiplier.
#pragma once
#include "msm_types.hpp"

namespace bh {
MsmJobImpl *msm_job_new(Context *ctx, int group);
void msm_job_delete(MsmJobImpl *j);
int msm_job_enqueue(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                    const u64 *density_dev, const MsmOpts &opts);
int msm_job_finish(MsmJobImpl &job, void *out_affine, float *ms, u64 *stats8 = nullptr);
int msm_job_finish_many(MsmJobImpl &job, void *out_affine_k, size_t k, float *ms, u64 *stats8, bool *fallback);
int msm_debug_stages(Context &c, const void *scalars_host, u64 n, int fmt, unsigned cbits, u64 *pairs_out, u32 *zstart_out);
void msm_job_track(MsmJobImpl &job);
int msm_job_start(MsmJobImpl &job);
bool msm_slot_try_reserve(Context &c);
void msm_slot_release(Context &c);
bool msm_complete_oldest(Context &c);
size_t msm_jobs_in_flight(Context &c);
hipStream_t msm_job_stream(MsmJobImpl &job);
int msm_job_after(MsmJobImpl &job, hipStream_t after);
void msm_job_set_result(MsmJobImpl &job, int rc, const void *affine_record);
void msm_job_own(MsmJobImpl &job, void *dev_ptr);
int fixed_base_mul(int group, const void *base_host, const void *scalars_dev, u64 n, int fmt, void *out_dev,
                   hipStream_t st, void *table_dev);
}  // namespace bh
