"""k Fr transforms (and k h blocks) of one size: the k calls a caller can make today against the batched call
(bh_fft_fr_many_dev, bh_h_poly_fr_many_dev_on), the measurement the dispatch rule of api_domain.hip (fft_many_wins) is set from.

Method: host wall time from the first issue to a final stream synchronisation, min of REPS repetitions after one warm-up
round, the three variants interleaved in one process (A B C A B C ...), the same device-resident inputs for every variant,
regenerated on the device before every timed call (bh_fr_powers_dev, outside the timed region).
  baseline  transforms: k calls of bh_fft_fr_dev; h block: k calls of bh_h_poly_fr_dev_on on one stream (existing code)
  many      the batched call with BH_FFT_MANY_FORCE
  default   the batched call with flags 0 (the dispatch rule)
Shapes: log_n = 6 ... 22 in steps of 2, k in {2, 4, 16, 64} with k * 2^log_n <= 2^24; ifft at every k, the four modes at one
k per size, and the h block at every k.  A shape's batched call "wins" when
min(many) < min(baseline) - (max(baseline) - min(baseline)): the baseline's own spread in this run is the margin.

Usage: python tools/bench_fft_many.py [--out profiles/fft_many_bench.json] [--reps 5] [--max-log-n 22]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("fft", "ifft", "coset_fft", "icoset_fft")
FORCE = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_many_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-log-n", type=int, default=6)
    ap.add_argument("--max-log-n", type=int, default=22)
    ap.add_argument("--ks", default="2,4,16,64")
    ap.add_argument("--all-modes-k", type=int, default=4)
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd.groth16 import fr_to_mont_array

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    ctx = worker.ctx
    at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    gens = fr_to_mont_array([0x9E3779B97F4A7C15, 3, 0xC2B2AE3D27D4EB4F, 5, 0x165667B19E3779F9, 7])

    def fill(dev, count, which):   # count elements of scale * g^i: the same inputs before every timed call
        assert lib.bh_fr_powers_dev(ctx, dev, count, p(gens[2 * which: 2 * which + 1]), p(gens[2 * which + 1: 2 * which + 2]), None) == 0

    rows = []
    for log_n in range(args.min_log_n, args.max_log_n + 1, 2):
        n = 1 << log_n
        vec = n * 32
        ks = [k for k in (int(x) for x in args.ks.split(",")) if k * n <= 1 << 24]
        kmax = max(ks)
        bufs = [worker.alloc(kmax * vec) for _ in range(3)]
        scratch = worker.alloc(kmax * vec)

        def sample(k):   # the first two elements of vector 0 and the last two of vector k - 1: the variants agree
            out = np.empty((4, 4), dtype=np.uint64)
            worker.download(out[:2], bufs[0])
            worker.download(out[2:], at(bufs[0], k * vec - 64))
            return out

        for k in ks:
            shapes = [("transform", m) for m in range(4) if m == 1 or k == min(args.all_modes_k, kmax)] + [("h_block", None)]
            for what, mode in shapes:
                if what == "transform":
                    def baseline():
                        for j in range(k):
                            assert lib.bh_fft_fr_dev(ctx, at(bufs[0], j * vec), log_n, mode, None) == 0

                    def many(flags):
                        assert lib.bh_fft_fr_many_dev(ctx, bufs[0], vec, k, log_n, mode, flags, None) == 0
                else:
                    def baseline():
                        for j in range(k):
                            assert lib.bh_h_poly_fr_dev_on(ctx, at(bufs[0], j * vec), at(bufs[1], j * vec), at(bufs[2], j * vec), scratch,
                                                           log_n, None) == 0

                    def many(flags):
                        assert lib.bh_h_poly_fr_many_dev_on(ctx, bufs[0], bufs[1], bufs[2], vec, k, log_n, flags, scratch, k * vec, None) == 0
                variants = (("baseline", baseline), ("many", lambda: many(FORCE)), ("default", lambda: many(0)))
                times = {name: [] for name, _ in variants}
                seen = {}
                for rep in range(args.reps + 1):
                    for name, fn in variants:
                        for i in range(3 if what == "h_block" else 1):
                            fill(bufs[i], k * n, i)
                        worker.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        worker.synchronize()
                        if rep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                        seen[name] = sample(k)
                assert np.array_equal(seen["baseline"], seen["many"]) and np.array_equal(seen["baseline"], seen["default"])
                b, m, d = times["baseline"], times["many"], times["default"]
                spread = max(b) - min(b)
                row = {"what": what if what == "h_block" else MODES[mode], "log_n": log_n, "k": k,
                       "baseline_ms": [round(x, 4) for x in b], "many_ms": [round(x, 4) for x in m], "default_ms": [round(x, 4) for x in d],
                       "baseline_min": round(min(b), 4), "baseline_spread": round(spread, 4), "many_min": round(min(m), 4),
                       "default_min": round(min(d), 4), "ratio_baseline_over_many": round(min(b) / min(m), 3),
                       "many_wins": bool(min(m) < min(b) - spread), "default_ok": bool(min(d) <= min(b) + spread)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        for d in bufs + [scratch]:
            worker.free(d)
        worker.trim()
    info = worker.info()
    out = {"tool": "tools/bench_fft_many.py",
           "method": "host wall ms from first issue to a final stream sync, min of %d reps after one warm-up round, variants "
                     "interleaved in one process, inputs regenerated on the device before every timed call" % args.reps,
           "not_measured": "kernel time by rocprofv3, any share of peak",
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
