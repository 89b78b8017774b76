"""Per-proof verdicts for many Groth16 proofs in one call (bh_groth16_verify_each, csrc/pairing.hip) against the two ways the
library had before it: bh_groth16_verify proof by proof, and bh_groth16_batch_verify (one verdict for the whole batch).

Writes profiles/verify_each_bench.json.  Fixture as tools/bench_verify.py: MiMC-322 proofs re-randomised into as many valid
proofs as a call needs; for the 16-input figures the key's ic gets 15 further points and the inputs are random, so every
proof fails its pairing check after exactly the work of a valid one.  All wall times are host clocks around synchronous
calls (each ends in a stream synchronisation), the median over --reps after one warm-up call per shape.

  python tools/bench_verify_each.py [--reps K] [--out FILE]
      proofs/s at 2^10, 2^14, 2^16 proofs with 1 and 16 inputs; bh_groth16_batch_verify at the same sizes; 64 sequential
      bh_groth16_verify calls; the 2^14 call with one shared-squaring three-pair Miller loop per proof instead of the
      shipped three one-pair loops (BELLMAN_HIP_VERIFY_EACH_SHARED=1, read once per process: measured in child
      processes, alternating with children that run the shipped form).  Exits 1 when verify_each over 2^14 proofs does
      not take less wall time than the 64 single calls.
  python tools/bench_verify_each.py --quick [--shared]
      one 2^14-proof call with 1 input and one with 16: the run to put under `rocprofv3 --kernel-trace --stats`
      (no counters in that run), e.g.
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ve -- python tools/bench_verify_each.py --quick
  python tools/bench_verify_each.py --merge DIR [--merge-shared DIR2] [--out FILE]
      adds the per-kernel times of those runs to the JSON"""

import argparse
import csv
import ctypes
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "verify_each_bench.json")

# Fp products per proof, counted as tools/bench_verify.py counts them
F12_SQR, LINE_MUL, F12_MUL = 36, 43, 54
MILLER_SHARED = 62 * F12_SQR + 3 * 68 * LINE_MUL
MILLER_SEPARATE = 3 * (62 * F12_SQR + 68 * LINE_MUL) + 2 * F12_MUL


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a


def setup():
    import bench_verify as bv
    import bellman_amd
    from bellman_amd import _lib, verifier

    lib = _lib.load()
    w = bellman_amd.Worker(0)
    params, proofs, images = bv.fixture(w)
    pvk = verifier.prepare_verifying_key(params)
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    pvk16 = verifier.PreparedVerifyingKey.from_elements(w, alpha_g1, beta_g2, gamma_g2, delta_g2,
                                                        np.concatenate([ic, np.tile(ic[1], (15, 1))]))
    return bv, lib, w, pvk, pvk16, proofs, images


def inputs_for(n, images_of_rows):
    from bellman_amd import verifier

    rnd = random.Random(1)
    ins1 = np.frombuffer(verifier._fr_bytes(images_of_rows), dtype=np.uint8).copy()
    ins16 = np.frombuffer(b"".join(rnd.randrange(verifier.Q).to_bytes(32, "little") for _ in range(16 * n)), dtype=np.uint8).copy()
    z = np.frombuffer(b"".join(rnd.randrange(1, verifier.Q).to_bytes(32, "little") for _ in range(n)), dtype=np.uint8).copy()
    return ins1, ins16, z


def time_each(lib, key, recs, n, inputs, n_in, want_bad, reps):
    verdicts = np.zeros(n, dtype=np.int32)
    n_bad = ctypes.c_size_t(0)
    ts = []
    for i in range(reps + 1):   # the first call warms the shape up (and builds the key's table once)
        t0 = time.perf_counter()
        rc = lib.bh_groth16_verify_each(key._h, _p(recs), n, _p(inputs), n_in, 0, _p(verdicts), ctypes.byref(n_bad))
        dt = time.perf_counter() - t0
        assert rc == 0 and n_bad.value == want_bad, (n, n_in, rc, n_bad.value)
        if i:
            ts.append(dt)
    return statistics.median(ts)


def quick(shared):
    if shared:
        os.environ["BELLMAN_HIP_VERIFY_EACH_SHARED"] = "1"   # read once, at the library's first call
    bv, lib, w, pvk, pvk16, proofs, images = setup()
    n = 1 << 14
    recs, ins = bv.rerandomised(w, proofs, images, n)
    ins1, ins16, _ = inputs_for(n, ins)
    t1 = time_each(lib, pvk, recs, n, ins1, 1, 0, 1)
    t16 = time_each(lib, pvk16, recs, n, ins16, 16, n, 1)
    pvk16.release()
    pvk.release()
    w.close()
    print(json.dumps({"shared": bool(shared), "n": n, "inputs1_s": t1, "inputs16_s": t16}))


def child_2p14(shared, reps):
    """the 2^14-proof call in a process of its own (the switch is read once per process) -> seconds, 1 and 16 inputs"""
    env = dict(os.environ)
    env.pop("BELLMAN_HIP_VERIFY_EACH_SHARED", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)] + (["--shared"] if shared else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def child(shared, reps):
    if shared:
        os.environ["BELLMAN_HIP_VERIFY_EACH_SHARED"] = "1"
    bv, lib, w, pvk, pvk16, proofs, images = setup()
    n = 1 << 14
    recs, ins = bv.rerandomised(w, proofs, images, n)
    ins1, ins16, _ = inputs_for(n, ins)
    out = {"shared": bool(shared), "inputs1_s": time_each(lib, pvk, recs, n, ins1, 1, 0, reps),
           "inputs16_s": time_each(lib, pvk16, recs, n, ins16, 16, n, reps)}
    pvk16.release()
    pvk.release()
    w.close()
    print(json.dumps(out))


def run(reps, out):
    from bellman_amd import _lib

    bv, lib, w, pvk, pvk16, proofs, images = setup()
    res = {"tool": "bench_verify_each", "library": _lib.library_identity(), "reps": reps,
           "what": "wall seconds of synchronous calls, median over reps after one warm-up call per shape",
           "fp_products_per_proof_counted": {"miller_shared": MILLER_SHARED, "miller_three_loops_and_two_products": MILLER_SEPARATE,
                                             "ratio": MILLER_SHARED / MILLER_SEPARATE}}
    sizes = [1 << 10, 1 << 14, 1 << 16]
    recs, ins = bv.rerandomised(w, proofs, images, max(sizes))
    ins1, ins16, z = inputs_for(max(sizes), ins)
    # 64 sequential bh_groth16_verify calls: the only way to per-proof verdicts before this entry point
    for i in range(3):
        assert lib.bh_groth16_verify(pvk._h, _p(recs[i]), _p(ins1[32 * i:]), 1, 0) == 0
    t0 = time.perf_counter()
    for i in range(64):
        assert lib.bh_groth16_verify(pvk._h, _p(recs[i]), _p(ins1[32 * i:]), 1, 0) == 0
    seq64 = time.perf_counter() - t0
    res["verify_proof_64_sequential_s"] = seq64
    each, batch = {}, {}
    for n in sizes:
        for n_in, key, inputs, bad, brc in ((1, pvk, ins1, 0, 0), (16, pvk16, ins16, n, 9)):
            t = time_each(lib, key, recs, n, inputs, n_in, bad, reps)
            each["n%d_inputs%d" % (n, n_in)] = {"seconds": t, "proofs_per_s": n / t}
            ts = []
            for i in range(reps + 1):
                t0 = time.perf_counter()
                rc = lib.bh_groth16_batch_verify(key._h, _p(recs), n, _p(inputs), n_in, 0, _p(z))
                if i:
                    ts.append(time.perf_counter() - t0)
                assert rc == brc, (n, n_in, rc)
            tb = statistics.median(ts)
            batch["n%d_inputs%d" % (n, n_in)] = {"seconds": tb, "proofs_per_s": n / tb, "verify_each_over_batch": t / tb}
    res["verify_each"], res["batch_verify"] = each, batch
    t14 = each["n%d_inputs1" % (1 << 14)]["seconds"]
    res["condition"] = {"what": "verify_each over 2^14 proofs takes less wall time than 64 sequential bh_groth16_verify calls",
                        "verify_each_2p14_s": t14, "verify_proof_64_sequential_s": seq64, "met": t14 < seq64}
    pvk16.release()
    pvk.release()
    w.close()
    # the Miller form: children alternate the shared-squaring loop and the shipped three one-pair loops (same box, same run)
    kids = [child_2p14(shared, reps) for shared in (True, False, True, False)]
    sh = [k for k in kids if k["shared"]]
    se = [k for k in kids if not k["shared"]]
    form = {}
    for key in ("inputs1_s", "inputs16_s"):
        a, b = statistics.median(k[key] for k in sh), statistics.median(k[key] for k in se)
        form[key] = {"shared_squarings": a, "three_loops_and_two_products": b, "shared_over_separate": a / b,
                     "all": [("shared" if k["shared"] else "three_loops", k[key]) for k in kids]}
    res["miller_form_2p14_call"] = form
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["condition"]["met"] else 1


def kernel_table(d):
    kern = {}

    def put(name, calls, total_ns, max_ns, min_ns):
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("bh::", "").strip()
        k = kern.setdefault(short, {"calls": 0, "total_ms": 0.0, "longest_launch_ms": 0.0, "shortest_launch_ms": 1e30})
        k["calls"] += int(calls)
        k["total_ms"] += float(total_ns) / 1e6
        k["longest_launch_ms"] = max(k["longest_launch_ms"], float(max_ns) / 1e6)
        k["shortest_launch_ms"] = min(k["shortest_launch_ms"], float(min_ns) / 1e6)

    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            put(r["Name"], r["Calls"], r["TotalDurationNs"], r["MaxNs"], r["MinNs"])
    if not kern:
        import sqlite3

        for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
            db = sqlite3.connect(f)
            for name, calls, total, mx, mn in db.execute("select name, count(*), sum(end - start), max(end - start), min(end - start) "
                                                          "from kernels group by name"):
                put(name, calls, total, mx, mn)
    assert kern, "no kernel statistics under %s" % d
    return {k: {kk: (round(vv, 3) if isinstance(vv, float) else vv) for kk, vv in v.items()}
            for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["total_ms"])}


STAGES = (("ic_accumulation", ("ic_accumulate_kernel",)), ("g2_lines", ("g2_lines_kernel",)), ("miller_three_pairs", ("miller3_kernel",)),
          ("final_exponentiation_chain", ("fe_easy_kernel", "fe_mul_op_kernel", "fe_cyc_sqr_kernel", "fe_conj_kernel", "fe_finish_kernel")),
          ("curve_checks", ("proof_prep_kernel",)), ("constant_and_products", ("f12_mul_const_kernel", "f12_fold_kernel")),
          ("verdicts", ("verdict_kernel",)), ("key_table_once", ("ic_table_kernel", "miller_kernel")))


def merge(d, d_shared, out):
    """the --quick run under the kernel trace makes four 2^14-proof calls: a warm-up and a timed one with 1 input, then
    the same with 16 - so a stage's time per 2^14 chunk is its total over four (the accumulation: shortest launch for 1
    input, longest for 16)"""
    with open(out) as f:
        doc = json.load(f)
    for tag, dd in (("kernel_trace_2p14", d), ("kernel_trace_2p14_shared_squarings", d_shared)):
        if not dd:
            continue
        kern = kernel_table(dd)
        stages = {}
        for stage, names in STAGES:
            got = [kern[n] for n in names if n in kern]
            stages[stage] = {"launches": sum(g["calls"] for g in got), "total_ms": round(sum(g["total_ms"] for g in got), 3),
                             "per_chunk_ms": round(sum(g["total_ms"] for g in got) / 4, 3)}
        if "ic_accumulate_kernel" in kern:
            stages["ic_accumulation"]["inputs1_ms"] = kern["ic_accumulate_kernel"]["shortest_launch_ms"]
            stages["ic_accumulation"]["inputs16_ms"] = kern["ic_accumulate_kernel"]["longest_launch_ms"]
        doc[tag] = {"chunks": 4, "stages": stages, "kernels": kern}
    b, a = doc.get("kernel_trace_2p14"), doc.get("kernel_trace_2p14_shared_squarings")
    if a and b:
        ta = a["stages"]["miller_three_pairs"]["per_chunk_ms"]
        tb = b["stages"]["miller_three_pairs"]["per_chunk_ms"] + b["stages"]["constant_and_products"]["per_chunk_ms"] - \
            a["stages"]["constant_and_products"]["per_chunk_ms"]
        doc["miller_form_kernel_time_2p14"] = {"shared_squarings_ms": ta, "three_loops_and_two_products_ms": round(tb, 3),
                                               "measured_ratio": round(ta / tb, 3), "counted_ratio": round(MILLER_SHARED / MILLER_SEPARATE, 3)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in doc if k.startswith("miller_form") or k == "condition"}, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shared", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--merge-shared", default=None)
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.merge_shared, a.out)
    elif a.quick:
        quick(a.shared)
    elif a.child:
        child(a.shared, a.reps)
    else:
        sys.exit(run(a.reps, a.out))
