// G1 (Fp) instantiation of the MSM pipeline: one lane per point (a single kernel bundle: no flag, no size switch)
#include "msm_ec.cuh"
namespace bh {
int msm_enqueue_g1(MsmJobImpl &job, const MsmBases &bases, u64 skip, const void *scalars_dev, u64 n, int fmt,
                   const u64 *density_dev, const MsmOpts &opts) {
  return msm_enqueue<FpOps, FpOps>(job, bases, skip, scalars_dev, n, fmt, density_dev, opts);
}
BH_INSTANTIATE_MSM_SUPPORT(g1, FpOps)
}
