"""Times the pieces of a powers-of-tau check on the GPU and writes profiles/ptau_verify_bench.json.

For 2^16, 2^18 and 2^20 points per group (tau_g1 holds twice as many) it records, as host wall time around calls that end
in a device synchronise (minimum and median over --reps after one warm-up call):
  validate   bh_bases_validate(CHECKED | FORBID_IDENTITY) over the resident tau_g1 and tau_g2, per point, beside
             bh_bases_read_uncompressed with the same flags on the same points - the [q] P path it is an alternative to -
             in one process, the repetitions interleaved (validate, reader, upload, validate, ...).  The reader also
             uploads its bytes and registers a handle: the upload alone is timed too, and automatic window tables are switched off in this part (BELLMAN_HIP_TABLE_MAX_LOG2=0) so that no
             table build is inside the reader's time.
  verify     bh_powers_of_tau_verify without BH_PTAU_VALIDATE_POINTS on a consistent transcript (default registration, so
             the handles carry their automatic window tables), and the eight multiexps alone (bh_test_ptau_sums - the same
             function the check calls), interleaved; pairings = the difference.
Each part runs in a child process of its own, under a time limit (--part-timeout seconds).  No time here is a pass criterion.

Usage: python tools/bench_ptau_verify.py [--logs 16,18,20] [--reps 5] [--out profiles/ptau_verify_bench.json]"""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Fp products per point counted from the formulas (csrc/point_read.hip, ec.cuh; tools/bench_proof_read.py counts the same
# way: an Fp2 product is 3 Fp products, an Fp2 square 2)
G1_DBL, G1_MADD, G1_ADD, G2_DBL, G2_MADD = 9, 10, 14, 24, 28
PRODUCTS = {
    "g1_validate": 3 + 2 * 63 * G1_DBL + 5 * (G1_MADD + G1_ADD) + 3,   # on-curve, two mul_z, beta x and the comparison
    "g2_validate": 7 + 63 * G2_DBL + 5 * G2_MADD + 6 + 6,              # on-curve, one mul_z, the two psi products, the comparison
    "g1_q_test": 3621, "g2_q_test": 9835,                              # on-curve + [q] P
}
TAU, ALPHA, BETA = 0x1F3D5B79A2C4E6081, 0x2B7E151628AED2A6, 0x3243F6A8885A308D


def timed_interleaved(fns, reps):
    """one warm-up call of each, then `reps` rounds that call each function once in turn: what the host shares with
    others disturbs all of them alike"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [{"min_ms": min(t), "median_ms": statistics.median(t), "max_ms": max(t), "reps": reps} for t in ts]


def powers_bases(worker, group, n, scale):
    from bellman_amd import _lib
    from bellman_amd.errors import check
    from bellman_amd.groth16 import fr_to_mont_array
    from bellman_amd.multiexp import Bases
    from oracle import cref

    lib, ctx = _lib.load(), worker.ctx
    rec = 96 if group == 1 else 192
    sc, pts = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bh_dev_alloc(ctx, n * 32 + 32, ctypes.byref(sc)))
    check(lib.bh_dev_alloc(ctx, n * rec + rec, ctypes.byref(pts)))
    try:
        gs = fr_to_mont_array([TAU, scale])
        check(lib.bh_fr_powers_dev(ctx, sc, n, gs[0:1].ctypes.data_as(ctypes.c_void_p), gs[1:2].ctypes.data_as(ctypes.c_void_p), None))
        base = cref.g1_generator() if group == 1 else cref.g2_generator()
        check(lib.bh_fixed_base_mul_dev(ctx, group, base.ctypes.data_as(ctypes.c_void_p), sc, n, 1, pts, None))
        return Bases.copy_device(worker, group, pts, n)
    finally:
        lib.bh_dev_free(ctx, sc)
        lib.bh_dev_free(ctx, pts)


def part_validate(logs, reps):
    import numpy as np

    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd.errors import check

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    ctx = worker.ctx
    out = []
    for lg in logs:
        for group, n in ((1, 2 << lg), (2, 1 << lg)):
            rec = 96 if group == 1 else 192
            bases = powers_bases(worker, group, n, 1)
            raw = np.zeros(n * rec, dtype=np.uint8)
            check(lib.bh_bases_write_uncompressed(ctx, bases._h, 0, n, raw.ctypes.data_as(ctypes.c_void_p)))
            dev = ctypes.c_void_p()
            check(lib.bh_dev_alloc(ctx, n * rec, ctypes.byref(dev)))

            def validate():
                check(lib.bh_bases_validate(ctx, bases._h, 0, n, 3, None, None))

            def reader():
                h = ctypes.c_void_p()
                check(lib.bh_bases_read_uncompressed(ctx, group, raw.ctypes.data_as(ctypes.c_void_p), n, 3, ctypes.byref(h), None))
                lib.bh_bases_release(ctx, h)

            def upload():
                check(lib.bh_dev_upload(ctx, dev, raw.ctypes.data_as(ctypes.c_void_p), n * rec))

            v, r, u = timed_interleaved([validate, reader, upload], reps)
            key = "g%d" % group
            out.append({"log_n": lg, "group": group, "points": n, "validate": v, "read_uncompressed_checked": r,
                        "upload_alone": u, "validate_ns_per_point": v["min_ms"] * 1e6 / n,
                        "reader_ns_per_point": r["min_ms"] * 1e6 / n,
                        "reader_minus_upload_ns_per_point": (r["min_ms"] - u["min_ms"]) * 1e6 / n,
                        "measured_ratio_reader_minus_upload_over_validate": (r["min_ms"] - u["min_ms"]) / v["min_ms"],
                        "counted_ratio_fp_products": PRODUCTS[key + "_q_test"] / PRODUCTS[key + "_validate"],
                        "validate_fp_products_per_s": PRODUCTS[key + "_validate"] * n / (v["min_ms"] * 1e-3)})
            lib.bh_dev_free(ctx, dev)
            bases.release()
    worker.close()
    return out


def part_verify(logs, reps):
    import numpy as np

    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd.ceremony import PtauReport, _PowersOfTau
    from oracle import cref

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    ctx = worker.ctx
    seed = bytes(range(32))
    out = []
    for lg in logs:
        n = 1 << lg
        vec = [powers_bases(worker, 1, 2 * n, 1), powers_bases(worker, 2, n, 1), powers_bases(worker, 1, n, ALPHA),
               powers_bases(worker, 1, n, BETA)]
        beta_g2 = cref.point_mul(2, cref.g2_generator(), BETA)
        t = _PowersOfTau(*[b._h for b in vec], beta_g2.ctypes.data)
        rep = PtauReport()
        sums = np.zeros((8, 24), dtype=np.uint64)
        rcs = (ctypes.c_int * 8)()

        def verify():
            rc = lib.bh_powers_of_tau_verify(ctx, ctypes.byref(t), seed, 0, ctypes.byref(rep))
            assert rc == 0 and rep.failed == 0, (rc, rep.failed)

        def multiexps():
            assert lib.bh_test_ptau_sums(ctx, ctypes.byref(t), seed, sums.ctypes.data_as(ctypes.c_void_p), rcs) == 0

        w, m = timed_interleaved([verify, multiexps], reps)
        out.append({"log_n": lg, "points": {"tau_g1": 2 * n, "tau_g2": n, "alpha_tau_g1": n, "beta_tau_g1": n},
                    "window_tables": [b.table_info() for b in vec], "verify_without_validation": w, "eight_multiexps": m,
                    "pairings_and_heads_ms_by_difference": w["min_ms"] - m["min_ms"]})
        for b in vec:
            b.release()
    worker.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_verify_bench.json"))
    ap.add_argument("--part", choices=["validate", "verify"])
    ap.add_argument("--part-timeout", type=float, default=300.0, help="seconds a child process may take")
    a = ap.parse_args()
    logs = [int(x) for x in a.logs.split(",")]
    if a.part:   # a child: one part, JSON on the last line of stdout
        from bellman_amd import _lib

        rows = (part_validate if a.part == "validate" else part_verify)(logs, a.reps)
        print(json.dumps({"library": _lib.library_identity(), "rows": rows}))
        return
    doc = {"tool": "bench_ptau_verify", "what": "host wall time around calls that end in a device synchronise, one warm-up call, "
           "min and median over reps; no number here is a pass criterion", "fp_products_per_point_counted": PRODUCTS}
    for part in ("validate", "verify"):
        env = dict(os.environ)
        if part == "validate":
            env["BELLMAN_HIP_TABLE_MAX_LOG2"] = "0"
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--logs", a.logs, "--reps", str(a.reps)],
                             env=env, capture_output=True, text=True, timeout=a.part_timeout)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit("part %s failed with %d: nothing written" % (part, res.returncode))
        got = json.loads(res.stdout.strip().splitlines()[-1])
        doc["library"], doc[part] = got["library"], got["rows"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
