"""Times the check of a circuit-specific ceremony step on the GPU and writes profiles/phase2_verify_bench.json.

For the chain circuit at 2^16, 2^18 and 2^20 constraints, with `after` = `before`.rescale_delta(d), it records as host wall
time around calls that end in a device synchronise (minimum and median over --reps interleaved repetitions after one
warm-up call of each):
  verify_step            bh_groth16_params_verify_step with and without BH_STEP_VALIDATE_POINTS
  four_multiexps         the sums over h, h', l, l' alone (bh_test_phase2_sums - the same function the check calls)
  three_comparisons      bh_bases_first_difference over a, b_g1 and b_g2 alone
  compare / memcpy       the comparison of the `a` queries alone, as bytes read per second, beside a device-to-device
                         hipMemcpyAsync of the same number of bytes (it reads half of them and writes the other half) timed
                         in the same rounds: the memcpy is the yardstick, the ratio is reported, there is no pass mark
  write_and_memcmp       the only alternative there was: bh_groth16_params_write of both sets and a comparison on the host
                         (which cannot tell a rescaled h from a wrong one; it is the cost of getting the bytes at all)
and bh_pairing_same_ratio_each at 2, 64 and 2048 rows.  Each part runs in a child process of its own, under a time limit
(--part-timeout seconds).  No time here is a pass criterion.

Usage: python tools/bench_phase2_verify.py [--logs 16,18,20] [--reps 5] [--out profiles/phase2_verify_bench.json]"""

import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ptau_verify import timed_interleaved  # noqa: E402

TOXIC = (0x2B7E151628AED2A6, 0x3243F6A8885A308D, 0x1F3D5B79A2C4E6081, 0x9E3779B97F4A7C15, 0x6A09E667F3BCC908)
D = 0xD1CE5EED5EED


def part_step(logs, reps):
    import numpy as np

    import bellman_amd
    from bellman_amd import _lib
    from bellman_amd import groth16 as pg
    from bellman_amd.errors import check
    from oracle import cref

    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    worker = bellman_amd.Worker(0)
    ctx = worker.ctx
    seed = bytes(range(32))
    out = []
    for lg in logs:
        r1cs = pg.R1CS.from_demo(worker, 1, (1 << lg) - 3, 2020)
        before = pg.Parameters.generate(worker, r1cs, cref.g1_generator(), cref.g2_generator(), *TOXIC)
        after = before.rescale_delta(D)
        rep = pg.ParamsStepReport()
        sums = np.zeros((4, 12), dtype=np.uint64)
        rcs = (ctypes.c_int * 4)()
        idx = ctypes.c_size_t()
        same = [(before.bases(q), after.bases(q)) for q in ("a", "b_g1", "b_g2")]
        lens = {q: len(before.bases(q)) for q in ("h", "l", "a", "b_g1", "b_g2")}
        n_a = lens["a"]
        src, dst = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.bh_dev_alloc(ctx, n_a * 96, ctypes.byref(src)))
        check(lib.bh_dev_alloc(ctx, n_a * 96, ctypes.byref(dst)))

        def step(flags):
            def run():
                rc = lib.bh_groth16_params_verify_step(ctx, before._h, after._h, seed, flags, ctypes.byref(rep))
                assert rc == 0 and rep.failed == 0, (rc, rep.failed)
            return run

        def multiexps():
            assert lib.bh_test_phase2_sums(ctx, before._h, after._h, seed, sums.ctypes.data_as(ctypes.c_void_p), rcs) == 0

        def comparisons():
            for x, y in same:
                assert lib.bh_bases_first_difference(ctx, x._h, 0, y._h, 0, len(x), ctypes.byref(idx)) == 0 and idx.value == len(x)

        def compare_a():
            assert lib.bh_bases_first_difference(ctx, same[0][0]._h, 0, same[0][1]._h, 0, n_a, ctypes.byref(idx)) == 0

        def memcpy():   # as many bytes as compare_a reads: n_a records read, n_a written
            assert hip.hipMemcpyAsync(dst, src, n_a * 96, 3, None) == 0 and hip.hipStreamSynchronize(None) == 0

        def write_and_memcmp():
            assert (before.write() == after.write()) is False

        names = ["verify_step", "verify_step_validate_points", "four_multiexps", "three_comparisons", "compare_a", "memcpy_d2d",
                 "write_and_memcmp"]
        ts = timed_interleaved([step(0), step(1), multiexps, comparisons, compare_a, memcpy, write_and_memcmp], reps)
        row = {"log_constraints": lg, "query_lengths": lens, "serialized_bytes_per_set": before.serialized_len()}
        row.update(dict(zip(names, ts)))
        moved = 2 * n_a * 96
        row["compare_a_bytes"] = moved
        row["compare_a_gb_per_s"] = moved / (row["compare_a"]["min_ms"] * 1e-3) / 1e9
        row["memcpy_d2d_gb_per_s"] = moved / (row["memcpy_d2d"]["min_ms"] * 1e-3) / 1e9
        row["compare_over_memcpy_time_ratio"] = row["compare_a"]["min_ms"] / row["memcpy_d2d"]["min_ms"]
        out.append(row)
        lib.bh_dev_free(ctx, src)
        lib.bh_dev_free(ctx, dst)
        after.release()
        before.release()
        r1cs.release()
    worker.close()
    return out


def part_same_ratio(rows_list, reps):
    import numpy as np

    import bellman_amd
    from bellman_amd.ceremony import same_ratio_each
    from oracle import cref

    worker = bellman_amd.Worker(0)
    g1, g2 = cref.g1_generator(), cref.g2_generator()
    three = [(3, 15, 7, 35), (5, 55, 9, 99), (3, 15, 7, 36)]   # two rows that hold and one that does not, repeated
    recs = [np.array([cref.point_mul(1 if k < 2 else 2, g1 if k < 2 else g2, r[k]) for r in three]) for k in range(4)]
    out = []
    for n in rows_list:
        pick = np.arange(n) % 3
        args = [np.ascontiguousarray(r[pick]) for r in recs]

        def run():
            v = same_ratio_each(worker, *args)
            assert int((v != 0).sum()) == int((pick == 2).sum())

        (t,) = timed_interleaved([run], reps)
        out.append({"rows": n, "same_ratio_each": t, "us_per_row": t["min_ms"] * 1e3 / n})
    worker.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20")
    ap.add_argument("--rows", default="2,64,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase2_verify_bench.json"))
    ap.add_argument("--part", choices=["step", "same_ratio"])
    ap.add_argument("--part-timeout", type=float, default=420.0, help="seconds a child process may take")
    a = ap.parse_args()
    if a.part:   # a child: one part, JSON on the last line of stdout
        from bellman_amd import _lib

        rows = part_step([int(x) for x in a.logs.split(",")], a.reps) if a.part == "step" else \
            part_same_ratio([int(x) for x in a.rows.split(",")], a.reps)
        print(json.dumps({"library": _lib.library_identity(), "rows": rows}))
        return
    doc = {"tool": "bench_phase2_verify", "what": "host wall time around calls that end in a device synchronise, one warm-up call, "
           "min and median over interleaved reps; no number here is a pass criterion"}
    for part in ("step", "same_ratio"):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--logs", a.logs, "--rows", a.rows,
                              "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.part_timeout)
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
