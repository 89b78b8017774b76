"""k proofs of one circuit from the values of the supplied variables alone: the call a user could make before
(prove_witness_batch(solver=..., check=True) on host buffers: upload, solve, download, upload, check, upload, prove) against
bh_groth16_prove_witness_batch_dev behind Solver.solve_many_dev on device buffers (one upload of the supplied values, then
solve -> check -> prove in place), with the proofs' tails finished on the host and on the device, and through the grouped path
(the test library's twin, mode 3 = BATCH_GROUPED_HE over the caller's buffers) with device finishing.  Separately:
bh_groth16_assemble_many against k calls of bh_groth16_assemble.  Witness path, synthetic CRS (distinct prime-order points:
timing only), the same values, r and s for every variant; the variants' proofs are compared.

Method (tools/bench_prove_batch.py's): host wall time, min of REPS repetitions, the variants interleaved in one process after
one warm-up round, every variant's own max - min spread recorded.  `device_finish_wins`: the device variant is ahead of the
host variant by more than the host variant's spread - the condition of the finish rule (groth16_batch.cpp
finish_on_device_by_rule), which needs it at every measured shape of a k.  `grouped_wins`: mode 3 with device finishing is
ahead of mode 0 with device finishing by more than that variant's spread - the same criterion for an automatic switch.

Usage: python tools/bench_prove_batch_dev.py [--out profiles/prove_batch_dev_bench.json] [--reps 5] [--ks 16,256]"""
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

from tests.circuits import boolmix_rounds  # noqa: E402
from tools.bench_prove_batch import Q, points  # noqa: E402

MIMC, CHAIN, BOOLMIX = 0, 1, 5
N_SUPPLIED = {MIMC: 2, CHAIN: 1, BOOLMIX: 64}


def timed(variants, reps):
    """min-of-reps wall ms per variant, interleaved, after one warm-up round -> ({name: [ms]}, {name: last result})"""
    results = {}
    for name, fn in variants:
        results[name] = fn()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t0 = time.perf_counter()
            results[name] = fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times, results


def stats(times):
    out = {}
    for name, t in times.items():
        out[name + "_min"] = round(min(t), 3)
        out[name + "_spread"] = round(max(t) - min(t), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch_dev_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="16,256")
    ap.add_argument("--assemble-ks", default="1,16,256,4096")
    ap.add_argument("--shapes", default="mimc-322,chain-2^14,chain-2^16,boolmix-2^16")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    rnd = random.Random(2025)
    ks = [int(x) for x in args.ks.split(",")]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    all_shapes = [("mimc-322", MIMC, 322, 0), ("chain-2^14", CHAIN, (1 << 14) - 3, 7), ("chain-2^16", CHAIN, (1 << 16) - 3, 7),
                  ("boolmix-2^16", BOOLMIX, boolmix_rounds(16), 7)]
    rows, params = [], None
    for name, kind, size, seed in [s for s in all_shapes if s[0] in args.shapes.split(",")]:
        cons = [rnd.randrange(Q) for _ in range(size)] if kind == MIMC else None
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
        n_sup = N_SUPPLIED[kind]
        solver = r1cs.solver([pg.Variable(pg.AUX, a) for a in range(n_sup)])
        kmax = max(ks)
        # buffers that hold nothing but ONE and the supplied values
        ins = np.zeros((kmax, n_in, 4), dtype=np.uint64)
        auxs = np.zeros((kmax, n_aux, 4), dtype=np.uint64)
        ins[:, 0] = pg.fr_to_mont_array([1])[0]
        vals = [rnd.randrange(2) if kind == BOOLMIX else rnd.randrange(Q) for _ in range(kmax * n_sup)]
        auxs[:, :n_sup] = pg.fr_to_mont_array(vals).reshape(kmax, n_sup, 4)
        rs = [rnd.randrange(Q) for _ in range(kmax)]
        ss = [rnd.randrange(Q) for _ in range(kmax)]
        for k in ks:
            ins_k, auxs_k = np.ascontiguousarray(ins[:k]), np.ascontiguousarray(auxs[:k])
            dw = pg.DeviceWitnesses.from_host(worker, ins_k, auxs_k)

            def host_entry():
                return pg.prove_witness_batch(r1cs, params, ins_k, auxs_k, rs[:k], ss[:k], solver=solver, check=True)

            def dev_entry(finish, mode=None):
                def run():
                    # the supplied values travel once; everything else happens where they land
                    assert lib.bh_dev_upload(worker.ctx, dw.inputs, p(ins_k), ins_k.nbytes) == 0
                    assert lib.bh_dev_upload(worker.ctx, dw.aux, p(auxs_k), auxs_k.nbytes) == 0
                    return pg.prove_witness_batch_dev(r1cs, params, dw, rs[:k], ss[:k], check=True, solver=solver, finish=finish,
                                                      _mode=mode)
                return run

            variants = [("host_entry", host_entry), ("dev_finish_host", dev_entry("host")), ("dev_finish_device", dev_entry("device")),
                        ("dev_mode3_finish_device", dev_entry("device", 3))]
            times, results = timed(variants, args.reps)
            same = all([q.write() for q in results[v]] == [q.write() for q in results["host_entry"]] for v, _ in variants)
            st = stats(times)
            row = {"circuit": name, "constraints": n_cons, "domain": m, "k": k, "proofs_equal": bool(same), **st,
                   "dev_finish_host_speedup_vs_host_entry": round(st["host_entry_min"] / st["dev_finish_host_min"], 3),
                   "dev_finish_device_speedup_vs_host_entry": round(st["host_entry_min"] / st["dev_finish_device_min"], 3),
                   "dev_entry_wins": bool(st["dev_finish_host_min"] < st["host_entry_min"] - st["host_entry_spread"]),
                   "device_finish_wins": bool(st["dev_finish_device_min"] < st["dev_finish_host_min"] - st["dev_finish_host_spread"]),
                   "dev_mode3_finish_device_speedup_vs_host_entry": round(st["host_entry_min"] / st["dev_mode3_finish_device_min"], 3),
                   "dev_mode3_vs_mode0_finish_device": round(st["dev_finish_device_min"] / st["dev_mode3_finish_device_min"], 3),
                   "grouped_wins": bool(st["dev_mode3_finish_device_min"] < st["dev_finish_device_min"] - st["dev_finish_device_spread"])}
            print(json.dumps(row), flush=True)
            rows.append(row)
            dw.release()
        solver.release()
        r1cs.release()
    # the proofs' tails alone: one device call against k host calls, over random sums
    asm = []
    for k in [int(x) for x in args.assemble_ks.split(",")]:
        g1 = points(worker, lib, 1, 6 * k, 21).reshape(k, 6, 12)
        g2 = points(worker, lib, 2, 2 * k, 22).reshape(k, 2, 24)
        sums = np.ascontiguousarray(np.concatenate([g1[:, :4].reshape(k, 48), g2.reshape(k, 48), g1[:, 4:].reshape(k, 24)], axis=1))
        r = pg.fr_to_mont_array([rnd.randrange(Q) for _ in range(k)])
        s = pg.fr_to_mont_array([rnd.randrange(Q) for _ in range(k)])

        def one_by_one():
            out = np.zeros((k, 48), dtype=np.uint64)
            for j in range(k):
                assert lib.bh_groth16_assemble(params._h, p(sums[j]), p(r[j]), p(s[j]), p(out[j])) == 0
            return out

        def many():
            out = np.zeros((k, 48), dtype=np.uint64)
            rcs = np.zeros(k, dtype=np.int32)
            assert lib.bh_groth16_assemble_many(params._h, p(sums), p(r), p(s), k, p(out), p(rcs)) == 0 and not rcs.any()
            return out

        times, results = timed([("assemble_k_calls", one_by_one), ("assemble_many", many)], args.reps if k < 4096 else 3)
        st = stats(times)
        row = {"k": k, "records_equal": bool(np.array_equal(results["assemble_k_calls"], results["assemble_many"])), **st,
               "assemble_many_speedup": round(st["assemble_k_calls_min"] / st["assemble_many_min"], 3),
               "per_proof_us_host": round(1e3 * st["assemble_k_calls_min"] / k, 1),
               "per_proof_us_device": round(1e3 * st["assemble_many_min"] / k, 1)}
        print(json.dumps(row), flush=True)
        asm.append(row)
    out = {"tool": "tools/bench_prove_batch_dev.py", "library": _lib.library_identity(),
           "method": "host wall ms, min of %d reps, variants interleaved in one process after a warm-up round; spread = max - min" % args.reps,
           "kernel_time_rocprofv3": "not measured", "k_above_256": "not measured", "rows": rows, "assemble": asm}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
