"""Index arithmetic of the sum kernel (bellman_amd/csrc/msm_sums.cuh, section 5c: nth_with_bit, partial_sum<WK>,
msm_sum_kernel<WK, NWAVES>) restated over any abelian group: plain integers in tests/test_bucket_sum_model_cpu.py, curve points
(tests/group_model.add, None = the identity) in tests/test_gpu_sum_jobs.py.  A job is a dict with the fields of SumDesc:
mode ("strided" / "bits"), groups, count, inner, stride, istride, group_shift, splits.  Everything is mirrored statement by
statement from the kernel, so a change there shows here."""
import operator


def nth_with_bit(j, k):   # msm_sums.cuh nth_with_bit
    return ((j >> k) << (k + 1)) | (1 << k) | (j & ((1 << k) - 1))


def partial_sum(d, data, g, sub, G, add=operator.add, zero=0):
    """what worker `sub` of the G workers of output g adds up (partial_sum<WK>)"""
    gg, ln = g // d["splits"], d["count"] // d["splits"]
    k0 = (g % d["splits"]) * ln
    outer, in_idx = gg // d["inner"], gg % d["inner"]
    base = outer << d["group_shift"]
    acc = zero
    if d["mode"] == "strided":
        for k in range(k0 + sub, k0 + ln, G):
            acc = add(acc, data[base + in_idx * d["istride"] + k * d["stride"]])
    else:   # bits: in_idx = bit position
        for j in range(sub, d["count"] >> 1, G):
            acc = add(acc, data[base + nth_with_bit(j, in_idx)])
    return acc


def run_job(d, data, G, add=operator.add, zero=0):
    out = []
    for g in range(d["groups"]):
        acc = zero
        for sub in range(G):
            acc = add(acc, partial_sum(d, data, g, sub, G, add, zero))
        out.append(acc)
    return out
