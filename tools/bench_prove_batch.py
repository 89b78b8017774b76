"""k proofs of one circuit: k sequential prove_witness calls, k prove_witness_async calls in flight, ONE
prove_witness_batch call (bh_groth16_prove_witness_batch) as shipped, and the same call through its grouped path (five
many-jobs per group of witnesses; the test library's twin of the call).  Witness path (constraint matrices resident), synthetic CRS
(distinct prime-order points: timing only), the same witnesses, r and s for every variant.

Method: host wall time of the k proofs, min of REPS repetitions, the variants interleaved in one process after one warm-up
round; the proofs of the three variants are compared.  The batch call is "ok" when its min is no slower than the better
baseline's by more than that baseline's own max - min spread.  The h blocks of the batch are k times the existing launches
(no batched FFT): `grouped_h_share` is the share of the grouped call's wall time that passes between the start of a group and
the issue of its last many-job - uploads, the k serial h blocks being enqueued, the issue of the jobs (the call's own
timings; the in-flight path has no such figure: its proofs overlap).  `grouped_wins`: the grouped path
beats the better baseline by more than that spread - the condition under which the call would take it.
`grouped_h`: the grouped path with a BATCHED h block (groth16.hpp BATCH_GROUPED_H: one bh_h_poly_fr_many_dev_on per group);
`grouped_h_share_batched` is the same share of its wall time, `grouped_h_wins` / `grouped_h_speedup_vs_best` as for the
grouped path.
`grouped_he`: BATCH_GROUPED_HE - the same with the group's constraint evaluations as ONE bh_r1cs_eval_many_dev and one upload
per vector kind; `grouped_he_vs_grouped_h` is the ratio of the two minima, `grouped_he_share_batched` the share as above.

Usage: python tools/bench_prove_batch.py [--out profiles/prove_batch_bench.json] [--reps 5] [--max-log 18]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import G1_GEN_MONT, G2_GEN_MONT, splitmix_scalars  # noqa: E402

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def points(worker, lib, group, n, seed):
    """n distinct prime-order points as host records (fixed-base multiples of the generator, computed on the device)"""
    words = 12 if group == 1 else 24
    gen = G1_GEN_MONT if group == 1 else G2_GEN_MONT
    dt, dout = worker.alloc(max(n, 1) * 32), worker.alloc(max(n, 1) * 8 * words)
    worker.upload(dt, splitmix_scalars(max(n, 1), seed))
    assert lib.bh_fixed_base_mul_dev(worker.ctx, group, gen.ctypes.data_as(ctypes.c_void_p), dt, n, 0, dout, None) == 0
    out = np.zeros((n, words), dtype=np.uint64)
    worker.download(out, dout)
    worker.free(dt)
    worker.free(dout)
    return out


def prove_one(lib, pg, r1cs, params, ia, aa, r, s):
    """bh_groth16_prove_witness over witness arrays that are already Montgomery"""
    rs = pg.fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.bh_groth16_prove_witness(params._h, r1cs._h, p(ia), ia.shape[0], p(aa), aa.shape[0], p(rs[0:1]), p(rs[1:2]), p(out), None) == 0
    return pg.Proof(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=18)
    ap.add_argument("--ks", default="4,16")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    rnd = random.Random(2024)
    ks = [int(x) for x in args.ks.split(",")]
    shapes = [("mimc-322", 0, 322, 0)] + [("chain-2^%d" % lg, 1, (1 << lg) - 3, 7) for lg in (14, 16, 18) if lg <= args.max_log]
    rows = []
    for name, kind, size, seed in shapes:
        cons = [rnd.randrange(Q) for _ in range(size)] if kind == 0 else None
        r1cs = pg.R1CS.from_demo(worker, kind, size, seed, cons)
        n_in, n_aux, n_cons = r1cs.num_inputs, r1cs.num_aux, r1cs.num_constraints
        m = 1
        while m < n_cons:
            m *= 2
        na = n_in + r1cs.density(0)[1]
        nb = r1cs.density(1)[1] + r1cs.density(2)[1]
        vk = [points(worker, lib, g, 1, 900 + i)[0] for i, g in enumerate((1, 1, 2, 1, 2))]
        params = pg.Parameters(worker, *vk, points(worker, lib, 1, m - 1, 11), points(worker, lib, 1, n_aux, 12),
                               points(worker, lib, 1, na, 13), points(worker, lib, 1, nb, 14), points(worker, lib, 2, nb, 15))
        kmax = max(ks)
        wits = []
        for j in range(kmax):
            w = [rnd.randrange(Q), rnd.randrange(Q)] if kind == 0 else [rnd.randrange(Q)]
            asg = pg.demo_assignment(kind, size, seed, w, cons)
            wits.append((asg["input_assignment"], asg["aux_assignment"]))
        rs = [rnd.randrange(Q) for _ in range(kmax)]
        ss = [rnd.randrange(Q) for _ in range(kmax)]
        for k in ks:
            def sequential():
                return [prove_one(lib, pg, r1cs, params, wits[j][0], wits[j][1], rs[j], ss[j]) for j in range(k)]

            def in_flight():
                jobs = [pg.prove_witness_async(r1cs, params, wits[j][0], wits[j][1], rs[j], ss[j]) for j in range(k)]
                return [w() for w in jobs]

            tm = [0, 0, 0, 0]
            # the batch call's own layout: witness j at row j of one array (built once, like the baselines' arrays)
            ins_k, auxs_k = np.stack([w[0] for w in wits[:k]]), np.stack([w[1] for w in wits[:k]])

            def batch():
                return pg.prove_witness_batch(r1cs, params, ins_k, auxs_k, rs[:k], ss[:k], tm)

            tm_g = [0, 0, 0, 0]

            def grouped():
                return pg.prove_witness_batch(r1cs, params, ins_k, auxs_k, rs[:k], ss[:k], tm_g, _workspace_budget=0)

            tm_h = [0, 0, 0, 0]

            def grouped_h():
                return pg.prove_witness_batch(r1cs, params, ins_k, auxs_k, rs[:k], ss[:k], tm_h, _workspace_budget=0, _mode=2)

            tm_he = [0, 0, 0, 0]

            def grouped_he():
                return pg.prove_witness_batch(r1cs, params, ins_k, auxs_k, rs[:k], ss[:k], tm_he, _workspace_budget=0, _mode=3)

            variants = (("sequential", sequential), ("async", in_flight), ("batch", batch), ("grouped", grouped), ("grouped_h", grouped_h),
                        ("grouped_he", grouped_he))
            times = {v: [] for v, _ in variants}
            res = {}
            for rep in range(args.reps + 1):
                for v, fn in variants:
                    t0 = time.perf_counter()
                    res[v] = fn()
                    if rep:
                        times[v].append((time.perf_counter() - t0) * 1e3)
            for j in range(k):
                for v in ("async", "batch", "grouped", "grouped_h", "grouped_he"):
                    assert all(np.array_equal(getattr(res[v][j], f), getattr(res["sequential"][j], f)) for f in "abc"), (name, k, v, j)
            best = min(("sequential", "async"), key=lambda v: min(times[v]))
            spread = max(times[best]) - min(times[best])
            row = {"circuit": name, "constraints": n_cons, "k": k,
                   **{v + "_ms": [round(x, 3) for x in times[v]] for v, _ in variants},
                   **{v + "_min": round(min(times[v]), 3) for v, _ in variants},
                   "best_baseline": best, "baseline_spread": round(spread, 3),
                   "batch_ok": bool(min(times["batch"]) <= min(times[best]) + spread),
                   "batch_speedup_vs_best": round(min(times[best]) / min(times["batch"]), 3),
                   "grouped_wins": bool(min(times["grouped"]) < min(times[best]) - spread),
                   "grouped_speedup_vs_best": round(min(times[best]) / min(times["grouped"]), 3),
                   "grouped_h_share": round(tm_g[1] / tm_g[3], 3) if tm_g[3] else None,
                   "grouped_h_wins": bool(min(times["grouped_h"]) < min(times[best]) - spread),
                   "grouped_h_speedup_vs_best": round(min(times[best]) / min(times["grouped_h"]), 3),
                   "grouped_h_vs_grouped": round(min(times["grouped"]) / min(times["grouped_h"]), 3),
                   "grouped_h_share_batched": round(tm_h[1] / tm_h[3], 3) if tm_h[3] else None,
                   "grouped_he_wins": bool(min(times["grouped_he"]) < min(times[best]) - spread),
                   "grouped_he_speedup_vs_best": round(min(times[best]) / min(times["grouped_he"]), 3),
                   "grouped_he_vs_grouped_h": round(min(times["grouped_h"]) / min(times["grouped_he"]), 3),
                   "grouped_he_share_batched": round(tm_he[1] / tm_he[3], 3) if tm_he[3] else None}
            rows.append(row)
            print(json.dumps(row), flush=True)
        params.release()
        r1cs.release()
        worker.trim()
    info = worker.info()
    out = {"tool": "tools/bench_prove_batch.py",
           "method": "host wall ms of k proofs, min of %d reps, variants interleaved in one process" % args.reps,
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
