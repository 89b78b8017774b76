"""The constraint evaluation and the satisfiability check for k witnesses of one circuit: the k bh_r1cs_eval_dev calls a caller
makes today against ONE bh_r1cs_eval_many_dev, bh_r1cs_check_many_dev beside it, and the checked batch prover
(bh_groth16_prove_witness_batch_checked) against the unchecked one - the price of the check pre-pass and its second upload.

Method: host wall time from the first issue to a final stream synchronisation, min of REPS repetitions after one warm-up
round, the variants interleaved in one process (A B C A B C ...), the same device-resident witnesses for every variant.
  eval_k     k calls of bh_r1cs_eval_dev into strided a, b, c vectors (existing code)
  eval_many  one bh_r1cs_eval_many_dev into the same vectors (compared with eval_k's, byte for byte, once per shape)
  check      one bh_r1cs_check_many_dev (every witness must come back satisfied)
The batched call "wins" when min(eval_many) < min(eval_k) - (max(eval_k) - min(eval_k)): the baseline's own spread in this
run is the margin.  Prover rows (host wall ms of the whole call, witnesses in the call's own layout, synthetic CRS):
  batch / checked   bh_groth16_prove_witness_batch / _checked; checked_over_batch is the ratio of their minima.
Shapes: MiMC-322 and the chain circuit at 2^14, 2^16, 2^18, 2^20 constraints, k = 4 and 16; the prover rows up to --prove-max-log.

Usage: python tools/bench_r1cs_many.py [--out profiles/r1cs_many_bench.json] [--reps 5] [--max-log 20] [--prove-max-log 18]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_prove_batch import points  # noqa: E402

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SATISFIED = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_many_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--prove-max-log", type=int, default=18)
    ap.add_argument("--ks", default="4,16")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    ctx = worker.ctx
    rnd = random.Random(2025)
    ks = [int(x) for x in args.ks.split(",")]
    at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
    shapes = [("mimc-322", 0, 322, 0, 0)] + [("chain-2^%d" % lg, 1, (1 << lg) - 3, 7, lg) for lg in (14, 16, 18, 20) if lg <= args.max_log]
    rows = []
    for name, kind, size, seed, lg in shapes:
        cons = [rnd.randrange(Q) for _ in range(size)] if kind == 0 else None
        r1cs = pg.R1CS.from_demo(worker, kind, size, seed, cons)
        n_in, n_aux, n_cons = r1cs.num_inputs, r1cs.num_aux, r1cs.num_constraints
        log_m = 0
        while (1 << log_m) < n_cons:
            log_m += 1
        vec = 32 << log_m
        kmax = max(ks)
        wits = []
        for j in range(kmax):
            w = [rnd.randrange(Q), rnd.randrange(Q)] if kind == 0 else [rnd.randrange(Q)]
            asg = pg.demo_assignment(kind, size, seed, w, cons)
            wits.append((asg["input_assignment"], asg["aux_assignment"]))
        ins, auxs = np.ascontiguousarray(np.stack([w[0] for w in wits])), np.ascontiguousarray(np.stack([w[1] for w in wits]))
        in_stride, aux_stride = n_in * 32, n_aux * 32
        d_in, d_aux = worker.alloc(ins.nbytes + 32), worker.alloc(auxs.nbytes + 32)
        worker.upload(d_in, ins)
        worker.upload(d_aux, auxs)
        outs = [worker.alloc(kmax * vec) for _ in range(3)]
        outs_k = [worker.alloc(kmax * vec) for _ in range(3)]
        d_bad = worker.alloc(kmax * 4)
        for k in ks:
            def eval_k():
                for j in range(k):
                    assert lib.bh_r1cs_eval_dev(ctx, r1cs._h, at(d_in, j * in_stride), at(d_aux, j * aux_stride), at(outs_k[0], j * vec),
                                                at(outs_k[1], j * vec), at(outs_k[2], j * vec), log_m, None) == 0

            def eval_many():
                assert lib.bh_r1cs_eval_many_dev(ctx, r1cs._h, d_in, in_stride, d_aux, aux_stride, k, outs[0], outs[1], outs[2], vec, log_m,
                                                 None) == 0

            def check():
                assert lib.bh_r1cs_check_many_dev(ctx, r1cs._h, d_in, in_stride, d_aux, aux_stride, k, d_bad, None) == 0

            variants = (("eval_k", eval_k), ("eval_many", eval_many), ("check", check))
            times = {v: [] for v, _ in variants}
            for rep in range(args.reps + 1):
                for v, fn in variants:
                    worker.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    worker.synchronize()
                    if rep:
                        times[v].append((time.perf_counter() - t0) * 1e3)
            got, want = np.empty(k * vec, dtype=np.uint8), np.empty(k * vec, dtype=np.uint8)
            for a, b in zip(outs, outs_k):
                worker.download(got, a)
                worker.download(want, b)
                assert np.array_equal(got, want), (name, k)
            bad = np.zeros(k, dtype=np.uint32)
            worker.download(bad, d_bad)
            assert (bad == SATISFIED).all(), (name, k, bad)
            b, m, c = times["eval_k"], times["eval_many"], times["check"]
            spread = max(b) - min(b)
            row = {"what": "eval", "circuit": name, "constraints": n_cons, "k": k,
                   **{v + "_ms": [round(x, 4) for x in times[v]] for v, _ in variants},
                   "eval_k_min": round(min(b), 4), "eval_k_spread": round(spread, 4), "eval_many_min": round(min(m), 4),
                   "check_min": round(min(c), 4), "ratio_eval_k_over_many": round(min(b) / min(m), 3),
                   "eval_many_wins": bool(min(m) < min(b) - spread), "ratio_check_over_eval_many": round(min(c) / min(m), 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        for d in [d_in, d_aux, d_bad] + outs + outs_k:
            worker.free(d)
        if lg <= args.prove_max_log:
            m = 1 << log_m
            na = n_in + r1cs.density(0)[1]
            nb = r1cs.density(1)[1] + r1cs.density(2)[1]
            vk = [points(worker, lib, g, 1, 900 + i)[0] for i, g in enumerate((1, 1, 2, 1, 2))]
            params = pg.Parameters(worker, *vk, points(worker, lib, 1, m - 1, 11), points(worker, lib, 1, n_aux, 12),
                                   points(worker, lib, 1, na, 13), points(worker, lib, 1, nb, 14), points(worker, lib, 2, nb, 15))
            rs = [rnd.randrange(Q) for _ in range(kmax)]
            ss = [rnd.randrange(Q) for _ in range(kmax)]
            for k in ks:
                tm = [0, 0, 0, 0]
                variants = (("batch", lambda: pg.prove_witness_batch(r1cs, params, ins[:k], auxs[:k], rs[:k], ss[:k])),
                            ("checked", lambda: pg.prove_witness_batch(r1cs, params, ins[:k], auxs[:k], rs[:k], ss[:k], tm, check=True)))
                times = {v: [] for v, _ in variants}
                res = {}
                for rep in range(args.reps + 1):
                    for v, fn in variants:
                        t0 = time.perf_counter()
                        res[v] = fn()
                        if rep:
                            times[v].append((time.perf_counter() - t0) * 1e3)
                for j in range(k):
                    assert all(np.array_equal(getattr(res["checked"][j], f), getattr(res["batch"][j], f)) for f in "abc"), (name, k, j)
                b, c = times["batch"], times["checked"]
                row = {"what": "prove", "circuit": name, "constraints": n_cons, "k": k, "batch_ms": [round(x, 3) for x in b],
                       "checked_ms": [round(x, 3) for x in c], "batch_min": round(min(b), 3), "batch_spread": round(max(b) - min(b), 3),
                       "checked_min": round(min(c), 3), "checked_over_batch": round(min(c) / min(b), 3),
                       "pre_pass_ms_last_call": round(tm[0], 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            params.release()
        r1cs.release()
        worker.trim()
    info = worker.info()
    out = {"tool": "tools/bench_r1cs_many.py",
           "method": "host wall ms from first issue to a final stream sync (eval rows) or of the whole call (prove rows), min of %d reps "
                     "after one warm-up round, variants interleaved in one process" % args.reps,
           "not_measured": "kernel time by rocprofv3, any share of peak",
           "witness_tile": int(lib.bh_test_r1cs_many_tile()),
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
