"""Times EvaluationDomain<Fr, Point<G>> transforms on the device (bh_fft_point_dev): G1 at 2^16, 2^18, 2^20 and G2 at
2^16, 2^18, fft and ifft, and writes profiles/point_fft_bench.json with, per case, the wall time of the call, the number
of non-trivial butterflies (twiddle != 1), the Fp products those butterflies execute under the fixed schedule of
csrc/point_fft.hip, and their share of the 40.08 G/s Fp-product ceiling (profiles/r1_microbench_int.txt).

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`:
    rocprofv3 --kernel-trace --stats -d DIR -o pf -- python tools/bench_point_fft.py --reps 1 --no-write
    python tools/bench_point_fft.py --merge DIR      (adds the per-kernel device times to the JSON)"""

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "point_fft_bench.json")

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ROOT_OF_UNITY = pow(7, (Q - 1) >> 32, Q)
CEILING = 40.08e9   # Fp products per second, profiles/r1_microbench_int.txt
# Fp products of the XYZZ formulas (ec.cuh): doubling, general addition; G2 counts its Fp2 products as 3 Fp (Karatsuba)
# and its squarings as 2
COST = {1: (9, 14), 2: (24, 40)}
CASES = [(1, 16), (1, 18), (1, 20), (2, 16), (2, 18)]


def butterfly_counts(group, log_n, inverse):
    """(non-trivial butterflies, Fp products): per stage of half-size m = 2^s the twiddles are omega^(j n/2m), j < m,
    each used by n/2m butterflies; [w]b costs (bits(w) - 1) doublings and (popcount(w) - 1) additions, and every
    butterfly adds two more additions"""
    dbl, add = COST[group]
    n = 1 << log_n
    w = pow(ROOT_OF_UNITY, 1 << (32 - log_n), Q)
    if inverse:
        w = pow(w, -1, Q)
    half = n // 2
    cost = np.zeros(half, dtype=np.int64)
    t = 1
    for i in range(half):
        cost[i] = dbl * (t.bit_length() - 1) + add * (bin(t).count("1") - 1) + 2 * add
        t = t * w % Q
    bfly, prods = 0, 0
    for s in range(log_n):
        lnb = log_n - 1 - s
        nb = 1 << lnb
        c = cost[:: nb][1: 1 << s]   # j = 1 .. m-1 (j = 0 is the trivial twiddle)
        bfly += nb * len(c)
        prods += nb * int(c.sum())
    return bfly, prods


def run(reps, write, out):
    import bellman_amd
    from oracle import cref
    from bellman_amd import _lib

    lib = _lib.load()
    w = bellman_amd.Worker(0)
    rows = []
    for group, log_n in CASES:
        n = 1 << log_n
        words = 12 if group == 1 else 24
        pts = cref.gen_bases(group, n, a=5, b=3)
        dev = w.alloc(n * words * 8)
        w.upload(dev, pts)
        for mode, name in ((0, "fft"), (1, "ifft")):
            assert lib.bh_fft_point_dev(w.ctx, group, dev, log_n, mode, None) == 0   # warm-up (tables, pool)
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                assert lib.bh_fft_point_dev(w.ctx, group, dev, log_n, mode, None) == 0
                times.append((time.perf_counter() - t0) * 1e3)
            bfly, prods = butterfly_counts(group, log_n, mode == 1)
            ms = min(times)
            row = {"group": "G%d" % group, "log_n": log_n, "mode": name, "ms": round(ms, 2), "ms_all": [round(t, 2) for t in times],
                   "nontrivial_butterflies": bfly, "fp_products": prods,
                   "fp_products_per_butterfly": round(prods / bfly, 1),
                   "time_at_ceiling_ms": round(prods / CEILING * 1e3, 2),
                   "share_of_ceiling": round(prods / CEILING * 1e3 / ms, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        w.free(dev)
    w.close()
    if write:
        doc = {"what": "bh_fft_point_dev wall time per call (min over reps, synchronous), tools/bench_point_fft.py",
               "ceiling_fp_products_per_s": CEILING, "reps": reps, "rows": rows}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


def merge(d, out):
    """per-kernel device time from the rocprofv3 --kernel-trace --stats run in directory d (its *kernel_stats.csv, or
    the kernels table of its rocpd database), added to the JSON"""
    kern = {}

    def put(name, calls, total_ns):
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("bh::", "")
        k = kern.setdefault(short, {"calls": 0, "total_ms": 0.0})
        k["calls"] += int(calls)
        k["total_ms"] += float(total_ns) / 1e6

    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            put(r["Name"], r["Calls"], r["TotalDurationNs"])
    if not kern:
        import sqlite3

        for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
            for name, calls, total in sqlite3.connect(f).execute(
                    "select name, count(*), sum(end - start) from kernels group by name"):
                put(name, calls, total)
    assert kern, "no kernel statistics under %s" % d
    with open(out) as f:
        doc = json.load(f)
    doc["kernel_stats"] = {k: {"calls": v["calls"], "total_ms": round(v["total_ms"], 2)} for k, v in
                           sorted(kern.items(), key=lambda kv: -kv[1]["total_ms"])}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernel_stats"], indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.out)
    else:
        run(a.reps, not a.no_write, a.out)
