"""Times the split-scalar point multiplier (bh_point_mul_each_dev, csrc/glv.cuh) against the ladder it would replace
(bh_point_mul_assign_dev, csrc/point_fft.hip) on the same points and the same per-point random scalars in the same
run - G1 at 2^16, 2^18, 2^20 points, G2 at 2^16, 2^18 - and a whole bh_powers_of_tau_contribute for m = 2^16, 2^18
(tau_g1 of 2m - 1 points, the other vectors of m).  Host wall time of the synchronous call, minimum of --reps
interleaved repetitions.  Writes profiles/point_mul_each_bench.json with the times, the ratios, the Fp products per
point counted over a sample of the scalars, and the two ratios the counts predict.

Every case runs in a child process under its own time limit; the first case that fails ends the run.
    python tools/bench_point_mul_each.py                  (on the GPU)
    python tools/bench_point_mul_each.py --resources      (anywhere: adds the kernels' register / scratch rows)"""

import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "point_mul_each_bench.json")

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF
# Fp products of the XYZZ formulas (ec.cuh): doubling, general addition, mixed addition; G2 counts an Fp2 product as 3 Fp
# and a squaring as 2; the G2 mixed addition of the split-scalar ladder recomputes its x coordinate (2 more)
COST = {1: {"dbl": 9, "add": 14, "madd": 10}, 2: {"dbl": 24, "add": 40, "madd": 30}}
MUL_CASES = [(1, 16), (1, 18), (1, 20), (2, 16), (2, 18)]
CONTRIBUTE_CASES = [16, 18]
CASE_LIMIT_S = 240


def random_scalars(n, seed):
    """[n, 4] uint64, uniform below 2^254 (< q); read as Montgomery form they are as uniform as read canonically"""
    sc = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2)
    sc += np.random.default_rng(seed + 1).integers(0, 2, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    return sc


def counted_products(group, sc_mont_sample):
    """Fp products per point of the two schedules for the scalars the kernels see (the canonical value behind each
    Montgomery word): the ladder doubles bits - 1 times and adds popcount - 1 times; the split-scalar ladder doubles
    from its first nonzero pair on and adds once per later nonzero pair"""
    c = COST[group]
    rinv = pow(1 << 256, -1, Q)
    ladder = glv = 0
    for row in sc_mont_sample:
        k = sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % Q
        ladder += c["dbl"] * (k.bit_length() - 1) + c["add"] * (bin(k).count("1") - 1)
        k1, k2 = k % LAMBDA, k // LAMBDA
        pairs = k1 | k2
        glv += c["dbl"] * (pairs.bit_length() - 1) + c["madd"] * (bin(pairs).count("1") - 1)
    return round(ladder / len(sc_mont_sample), 1), round(glv / len(sc_mont_sample), 1)


def mul_case(group, log_n, reps):
    import bellman_amd
    from bellman_amd import _lib
    from oracle import cref

    lib, w = _lib.load(), bellman_amd.Worker(0)
    n, words = 1 << log_n, 12 if group == 1 else 24
    pts = cref.gen_bases(group, n, a=5, b=3)
    sc = random_scalars(n, 100 * group + log_n)
    d_in, d_work, d_out, d_sc = w.alloc(pts.nbytes), w.alloc(pts.nbytes), w.alloc(pts.nbytes), w.alloc(sc.nbytes)
    w.upload(d_in, pts)
    w.upload(d_sc, sc)
    new_ms, old_ms = [], []
    for rep in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        assert lib.bh_point_mul_each_dev(w.ctx, group, d_in, d_sc, n, 1, d_out, None) == 0   # waits for the stream
        t1 = time.perf_counter()
        w.upload(d_work, pts)
        assert lib.bh_ctx_synchronize(w.ctx) == 0
        t2 = time.perf_counter()
        assert lib.bh_point_mul_assign_dev(w.ctx, group, d_work, d_sc, n, None) == 0
        assert lib.bh_ctx_synchronize(w.ctx) == 0
        t3 = time.perf_counter()
        if rep:
            new_ms.append((t1 - t0) * 1e3)
            old_ms.append((t3 - t2) * 1e3)
    got, want = np.zeros_like(pts), np.zeros_like(pts)
    w.download(got, d_out)
    w.download(want, d_work)
    assert np.array_equal(got, want), "the two multipliers disagree"
    for d in (d_in, d_work, d_out, d_sc):
        w.free(d)
    w.close()
    ladder, glv = counted_products(group, sc[:4096])
    return {"group": "G%d" % group, "log_n": log_n, "point_mul_each_ms": round(min(new_ms), 3), "ladder_ms": round(min(old_ms), 3),
            "ladder_over_point_mul_each": round(min(old_ms) / min(new_ms), 3),
            "point_mul_each_ms_all": [round(t, 3) for t in new_ms], "ladder_ms_all": [round(t, 3) for t in old_ms],
            "fp_products_per_point": {"ladder": ladder, "split_scalar": glv, "ratio": round(ladder / glv, 3)},
            "results_equal": True}


def contribute_case(log_m, reps):
    import bellman_amd
    from bellman_amd import ceremony

    w = bellman_amd.Worker(0)
    m = 1 << log_m
    start = ceremony.new_powers_of_tau(w, 2 * m - 1, m)
    challenge = {x: start.beta_g2 for x in ceremony.SECRETS}
    s = {x: start[0].download(0, 1)[0] for x in ceremony.SECRETS}
    times = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        after, _ = ceremony.contribute_powers_of_tau(w, start, 0x1234567 + rep, 0x89ABCDEF, 0x13579BDF, s, challenge)
        times.append((time.perf_counter() - t0) * 1e3)
        for b in after[:4]:
            b.release()
    w.close()
    return {"log_m": log_m, "points": {"G1": 4 * m - 1, "G2": m}, "contribute_ms": round(min(times[1:]), 2),
            "contribute_ms_all": [round(t, 2) for t in times[1:]],
            "note": "the whole call: four scale_powers with the registration of the new handles (window tables), beta_g2 on the host"}


def resources():
    """the register / scratch / occupancy rows clang reports for the kernels of point_mul.hip"""
    csrc = os.path.join(ROOT, "bellman_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "point_mul.hip", "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = {"kernel": re.sub(r"\(anonymous namespace\)::|bh::|void ", "", name).split("(")[0]}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=CASE_LIMIT_S)
    if out.returncode != 0:
        print(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("case %s failed (exit %d): nothing more is started" % (args, out.returncode))
    row = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--mul", nargs=2, type=int, default=None, help="child: one multiplication case (group, log_n)")
    ap.add_argument("--contribute", type=int, default=None, help="child: one contribution case (log_m)")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.mul:
        print(json.dumps(mul_case(a.mul[0], a.mul[1], a.reps)))
    elif a.contribute is not None:
        print(json.dumps(contribute_case(a.contribute, min(a.reps, 2))))
    elif a.resources:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_resources"] = resources()
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps(doc["kernel_resources"], indent=1))
    else:
        reps = ["--reps", str(a.reps)]
        rows = [child(["--mul", str(g), str(l)] + reps) for g, l in MUL_CASES]
        contrib = [child(["--contribute", str(l)] + reps) for l in CONTRIBUTE_CASES]
        doc = {"what": "bh_point_mul_each_dev against bh_point_mul_assign_dev: host wall time of the synchronous call, minimum of "
                       "%d interleaved repetitions, same points and per-point random scalars; tools/bench_point_mul_each.py" % a.reps,
               "predicted_by_the_counts": {"uniform_scalars": 1.9, "scalars_that_differ_per_lane": 2.4,
                                           "how": "G1: 4.07 k / 2.11 k Fp products per point; per wave-step 255 x (9 + 14) / (128 x (9 + 10))"},
               "rows": rows, "contribute": contrib}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
