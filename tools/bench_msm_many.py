"""k multiexps over one base vector: k ordinary jobs issued together against the many-plan (bh_msm_many_*), the
measurement the dispatch rule of api_msm.hip (many_plan_wins) is set from.

Method: host wall time from the first issue to the last result, min of REPS repetitions, the three variants interleaved
in one process (A B C A B C ...), the same registered bases (automatic window table where registration builds one) and
the same device-resident scalars for every variant, after one warm-up round.
  baseline  k bh_msm_async_dev_opts jobs issued together, then waited in order (existing code)
  many      bh_msm_many_async_dev with BH_MSM_MANY_FORCE
  default   bh_msm_many_async_dev as shipped (the dispatch rule)
plus, in a repetition of its own, the per-stage device times of the forced many-plan (BH_MSM_STAGE_TIMES).
A shape's many-plan "wins" when min(many) < min(baseline) - (max(baseline) - min(baseline)): the baseline's own spread in
this run is the margin.

Usage: python tools/bench_msm_many.py [--out profiles/msm_many_bench.json] [--g1-max 20] [--g2-max 18] [--reps 5]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import G1_GEN_MONT, G2_GEN_MONT, splitmix_scalars  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_many_bench.json"))
    ap.add_argument("--g1-max", type=int, default=20)
    ap.add_argument("--g2-max", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="2,4,8,16")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd.multiexp import MANY_FORCE

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    ks = [int(x) for x in args.ks.split(",")]
    kmax = max(ks)
    rows = []
    for group, top in ((1, args.g1_max), (2, args.g2_max)):
        for log_n in range(10, top + 1, 2):
            n = 1 << log_n
            words = 12 if group == 1 else 24
            gen = G1_GEN_MONT if group == 1 else G2_GEN_MONT
            dsc, dout = worker.alloc(kmax * n * 32), worker.alloc(n * 8 * words)
            worker.upload(dsc, splitmix_scalars(n, 0xB45E5 + group))
            assert lib.bh_fixed_base_mul_dev(worker.ctx, group, gen.ctypes.data_as(ctypes.c_void_p), dsc, n, 0, dout, None) == 0
            worker.synchronize()
            bases = bellman_amd.Bases.copy_device(worker, group, dout, n)
            worker.upload(dsc, splitmix_scalars(kmax * n, 0x5CA1A + group))
            table_bits = bases.table_info()[0]
            full = bellman_amd.FullDensity()

            def baseline(k):
                jobs = [bellman_amd.multiexp(worker, bases, full, None, scalars_dev=ctypes.c_void_p(dsc.value + v * n * 32), n=n)
                        for v in range(k)]
                return [j.wait() for j in jobs]

            def many(k, flags, stats=False):
                return bellman_amd.multiexp_many(worker, bases, full, None, scalars_dev=dsc, n=n, k=k, flags=flags, stats=stats).wait()

            for k in ks:
                variants = (("baseline", lambda: baseline(k)), ("many", lambda: many(k, MANY_FORCE)), ("default", lambda: many(k, 0)))
                times = {name: [] for name, _ in variants}
                results = {}
                for rep in range(args.reps + 1):
                    for name, fn in variants:
                        t0 = time.perf_counter()
                        results[name] = fn()
                        if rep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                for v in range(k):   # the variants agree
                    assert np.array_equal(results["baseline"][v], results["many"][v])
                    assert np.array_equal(results["baseline"][v], results["default"][v])
                _, ms, st = many(k, MANY_FORCE, stats=True)
                b, m, d = times["baseline"], times["many"], times["default"]
                spread = max(b) - min(b)
                row = {"group": "G%d" % group, "log_n": log_n, "k": k, "table_bits": table_bits,
                       "baseline_ms": [round(x, 4) for x in b], "many_ms": [round(x, 4) for x in m],
                       "default_ms": [round(x, 4) for x in d],
                       "baseline_min": round(min(b), 4), "baseline_spread": round(spread, 4), "many_min": round(min(m), 4),
                       "default_min": round(min(d), 4),
                       "many_wins": bool(min(m) < min(b) - spread), "default_ok": bool(min(d) <= min(b) + spread),
                       "many_device_ms": {"pipeline": round(ms[0], 4), "digits_sort": round(ms[1], 4),
                                          "bucket_accumulate": round(ms[2], 4), "merge_reduce": round(ms[3], 4)},
                       "many_plan": {"window_bits": st["window_bits"], "chunk": st["chunk"], "bucket_sets": st["bucket_sets"],
                                     "sorted_entries": st["sorted_entries"]}}
                rows.append(row)
                print(json.dumps(row), flush=True)
            bases.release()
            worker.free(dsc)
            worker.free(dout)
            worker.trim()
    info = worker.info()
    out = {"tool": "tools/bench_msm_many.py", "method": "host wall ms, min of %d reps, variants interleaved in one process" % args.reps,
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
