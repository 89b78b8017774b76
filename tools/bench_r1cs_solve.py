"""The witness solver (bh_r1cs_solve_many_dev) against what a caller does today: the circuit's value closures on one host
thread, once per witness.

Method (that of tools/bench_r1cs_many.py): host wall time from the issue of the call to a final stream synchronisation, min
of REPS repetitions after one warm-up round, the values of k interleaved in one process (k1 k4 k16 k256 k1 ...).  The
witnesses are device resident: buffers zeroed, then ONE and the supplied variables uploaded per witness - the solver
overwrites everything else.  After the timed runs the first witnesses are compared byte for byte with the host synthesis
(bh_test_demo_assignment) and bh_r1cs_check_many_dev must find every one of the k satisfied.
  baseline   k x bh_test_synthesis_ms(kind, size, seed, 3): the recycled WitnessAssignment on one host thread (min of 3 calls)
Shapes: MiMC-322, chain 2^14 / 2^16, boolean circuit 2^16 / 2^18 / 2^20 constraints; k = 1, 4, 16, 256.
No speed-up is asserted: the rows say what came out.
Sweep (--sweep): the two tuning words of csrc/r1cs_dev.hpp through bh_test_r1cs_solver_tune on chain 2^14 and the boolean
circuit at 2^16, k = 16 and 256: every level in the walk kernel at W = 1, 4, 16, 64 witnesses per workgroup, one launch per
level, and the automatic choice at switch points 2^14 ... 2^22 items.

Usage: python tools/bench_r1cs_solve.py [--out profiles/r1cs_solve_bench.json] [--reps 5] [--max-log 20] [--ks 1,4,16,256] [--sweep]"""
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

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SATISFIED = 0xFFFFFFFF
MIMC, CHAIN, BOOLMIX = 0, 1, 5
N_SUPPLIED = {MIMC: 2, CHAIN: 1, BOOLMIX: 64}
CHECKED = 3   # witnesses compared with the host synthesis


class Shape:
    def __init__(self, worker, lib, name, kind, size, seed, kmax, rnd):
        from bellman_amd import groth16 as pg

        self.worker, self.lib, self.name, self.kind, self.size, self.seed, self.kmax = worker, lib, name, kind, size, seed, kmax
        self.cons = [rnd.randrange(Q) for _ in range(size)] if kind == MIMC else None
        self.con_arr = pg.fr_to_mont_array(self.cons) if self.cons else None
        self.r1cs = pg.R1CS.from_demo(worker, kind, size, seed, self.cons)
        self.n_in, self.n_aux = self.r1cs.num_inputs, self.r1cs.num_aux
        t0 = time.perf_counter()
        self.solver = self.r1cs.solver([pg.Variable(pg.AUX, a) for a in range(N_SUPPLIED[kind])])
        self.create_ms = (time.perf_counter() - t0) * 1e3
        self.in_stride, self.aux_stride = self.n_in * 32, self.n_aux * 32
        self.d_in, self.d_aux = worker.alloc(kmax * self.in_stride + 32), worker.alloc(kmax * self.aux_stride + 32)
        self.d_bad = worker.alloc(kmax * 4)
        # the supplied values of kmax witnesses; the first CHECKED of them come from the host synthesis
        n_sup = N_SUPPLIED[kind]
        self.expect = []
        self.sup = np.zeros((kmax, n_sup, 4), dtype=np.uint64)
        for j in range(min(CHECKED, kmax)):
            w = [rnd.randrange(Q), rnd.randrange(Q)] if kind == MIMC else [rnd.randrange(Q)]
            asg = pg.demo_assignment(kind, size, seed, w, self.con_arr)
            self.expect.append((asg["input_assignment"], asg["aux_assignment"]))
            self.sup[j] = asg["aux_assignment"][:n_sup]
        for j in range(CHECKED, kmax):
            vals = [rnd.randrange(2) for _ in range(n_sup)] if kind == BOOLMIX else [rnd.randrange(Q) for _ in range(n_sup)]
            self.sup[j] = pg.fr_to_mont_array(vals)
        self.one = pg.fr_to_mont_array([1])

    def reset(self, k):
        """every slot zero but ONE and the supplied variables"""
        lib, ctx = self.lib, self.worker.ctx
        at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
        assert lib.bh_dev_zero(ctx, self.d_in, k * self.in_stride) == 0 and lib.bh_dev_zero(ctx, self.d_aux, k * self.aux_stride) == 0
        for j in range(k):
            assert lib.bh_dev_upload(ctx, at(self.d_in, j * self.in_stride), self.one.ctypes.data_as(ctypes.c_void_p), 32) == 0
            assert lib.bh_dev_upload(ctx, at(self.d_aux, j * self.aux_stride), self.sup[j].ctypes.data_as(ctypes.c_void_p), self.sup[j].nbytes) == 0
        self.worker.synchronize()

    def solve_ms(self, k):
        self.reset(k)
        t0 = time.perf_counter()
        assert self.lib.bh_r1cs_solve_many_dev(self.worker.ctx, self.solver._h, self.d_in, self.in_stride, self.d_aux, self.aux_stride, k, None) == 0
        self.worker.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def verify(self, k):
        """after a solve of k witnesses: the first ones byte for byte, all of them through the check"""
        at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
        for j, (want_in, want_aux) in enumerate(self.expect[:k]):
            got_in, got_aux = np.empty_like(want_in), np.empty_like(want_aux)
            self.worker.download(got_in, at(self.d_in, j * self.in_stride))
            self.worker.download(got_aux, at(self.d_aux, j * self.aux_stride))
            assert np.array_equal(got_in, want_in) and np.array_equal(got_aux, want_aux), (self.name, k, j)
        assert self.lib.bh_r1cs_check_many_dev(self.worker.ctx, self.r1cs._h, self.d_in, self.in_stride, self.d_aux, self.aux_stride, k,
                                               self.d_bad, None) == 0
        bad = np.zeros(k, dtype=np.uint32)
        self.worker.download(bad, self.d_bad)
        assert (bad == SATISFIED).all(), (self.name, k, bad)

    def tune(self, form=0, group=0, min_items=0):
        assert self.lib.bh_test_r1cs_solver_tune(self.solver._h, form, group, min_items) == 0

    def close(self):
        for d in (self.d_in, self.d_aux, self.d_bad):
            self.worker.free(d)
        self.solver.release()
        self.r1cs.release()
        self.worker.trim()


def interleaved(variants, reps):
    """variants: (label, fn -> ms) -> {label: [ms per rep]} after one warm-up round"""
    times = {label: [] for label, _ in variants}
    for rep in range(reps + 1):
        for label, fn in variants:
            ms = fn()
            if rep:
                times[label].append(round(ms, 4))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_solve_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--ks", default="1,4,16,256")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib

    lib = _lib.load().use_unchecked_demo_circuits()   # the baseline is the synthesis bench.py times
    worker = bellman_amd.Worker(0)
    rnd = random.Random(2026)
    ks = [int(x) for x in args.ks.split(",")]
    shapes = [("mimc-322", MIMC, 322, 0, 0)]
    shapes += [("chain-2^%d" % lg, CHAIN, (1 << lg) - 3, 7, lg) for lg in (14, 16) if lg <= args.max_log]
    shapes += [("boolmix-2^%d" % lg, BOOLMIX, boolmix_rounds(lg), 7, lg) for lg in (16, 18, 20) if lg <= args.max_log]
    rows, sweep = [], []
    for name, kind, size, seed, lg in shapes:
        sh = Shape(worker, lib, name, kind, size, seed, max(ks), rnd)
        host_ms = min(lib.bh_test_synthesis_ms(kind, size, seed, 3) for _ in range(3))
        times = interleaved([(k, lambda k=k: sh.solve_ms(k)) for k in ks], args.reps)
        for k in ks:
            sh.solve_ms(k)
            sh.verify(k)
            t = times[k]
            row = {"circuit": name, "constraints": sh.r1cs.num_constraints, "variables": sh.n_in + sh.n_aux, "k": k,
                   "plan": sh.solver.info, "solver_create_ms": round(sh.create_ms, 2), "solve_ms": t, "solve_min": min(t),
                   "solve_spread": round(max(t) - min(t), 4), "host_synthesis_ms_per_witness": round(host_ms, 4),
                   "baseline_ms": round(k * host_ms, 4), "ratio_baseline_over_solve": round(k * host_ms / min(t), 3),
                   "device_wins": bool(min(t) + (max(t) - min(t)) < k * host_ms)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        if args.sweep and name in ("chain-2^14", "boolmix-2^16"):
            for k in [x for x in (16, 256) if x <= max(ks)]:
                settings = [("walk W=%d" % w, (1, w, 0)) for w in (1, 4, 16, 64)] + [("level", (2, 0, 0))]
                settings += [("auto switch 2^%d" % e, (0, 0, 1 << e)) for e in (14, 16, 18, 20, 22)]

                def run(setting, k=k):
                    sh.tune(*setting)
                    ms = sh.solve_ms(k)
                    sh.tune()
                    return ms

                times = interleaved([(label, lambda s=s: run(s)) for label, s in settings], args.reps)
                row = {"circuit": name, "k": k, "min_ms": {label: min(t) for label, t in times.items()},
                       "spread_ms": {label: round(max(t) - min(t), 4) for label, t in times.items()}}
                sweep.append(row)
                print(json.dumps(row), flush=True)
        sh.close()
    info = worker.info()
    out = {"tool": "tools/bench_r1cs_solve.py",
           "method": "host wall ms from the issue of bh_r1cs_solve_many_dev to a final stream sync, min of %d reps after one warm-up "
                     "round, the values of k (the sweep: the settings) interleaved in one process; baseline = k x "
                     "bh_test_synthesis_ms(kind, size, seed, 3), min of 3" % args.reps,
           "not_measured": "kernel time by rocprofv3, any share of peak, the upload and download of the host form",
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(),
           "rows": rows, "sweep": sweep if args.sweep else "not measured"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
