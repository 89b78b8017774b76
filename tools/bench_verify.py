"""Groth16 verification on the device: verify_proof latency and batch::Verifier throughput (csrc/pairing.hip).

Prints one JSON line.  Fixture: generate_parameters for MiMC-322 (bellman's test circuit, one public input) and four proofs
of distinct preimages made on the device, re-randomised as (A / theta, B theta, C) into as many valid proofs as a batch
needs.  For the 16-input figures the key's ic gets 15 further points and the inputs are random: the proofs then no longer
verify, but every batch performs exactly the work of a valid one (the result is only read at the end).
Stage times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--quick).  There is no CPU pairing
on the machines this runs on, so there is no CPU baseline.

Usage: python tools/bench_verify.py [--quick] [--reps K] [--out FILE]
       python tools/bench_verify.py --merge BENCH_JSON KERNEL_STATS_CSV   (one JSON line: the bench line with the stage
                                                                            times of a --quick kernel-trace run added)"""

import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bellman_amd  # noqa: E402
from bellman_amd import _lib, verifier  # noqa: E402
from bellman_amd import groth16 as pg  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402  (the generators only)
from tests import circuits  # noqa: E402

Q = verifier.Q
P = bls.P


def _fp(v):
    return (v * (1 << 384) % P).to_bytes(48, "little")


# Fp products per proof, counted from the algorithm (csrc/fp12.cuh, csrc/pairing.hip; an Fp2 product is 3 Fp products
# (Karatsuba), an Fp2 square 2)
DBL_STEP = 3 * 3 + 6 * 2            # g2_dbl_step: 3 Fp2 products, 6 squares
ADD_STEP = 11 * 3 + 2 * 2           # g2_add_step
LINES = 63 * DBL_STEP + 5 * ADD_STEP
F12_SQR = 12 * 3                    # two Fp6 products
LINE_MUL = 13 * 3 + 4               # f12_mul_line + the two Fp2-by-Fp products with xP, yP
MILLER = 62 * F12_SQR + 68 * LINE_MUL
G1_DBL, G1_MADD, FP_INV = 9, 10, 381 + 190
Z_A = 256 * G1_DBL + 128 * G1_MADD + FP_INV + 4
F12_MUL = 54
PER_PROOF = {"g2_lines": LINES, "miller_loop": MILLER, "z_times_a": Z_A, "product": F12_MUL, "on_curve_checks": 2 * 3 + 3 * 3}
CEILING = 40.08e9   # Fp products/s, profiles/r1_microbench_int.txt


def fixture(worker):
    rnd = random.Random(2718)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    r1cs = pg.R1CS.from_demo(worker, 0, circuits.MIMC_ROUNDS, 0, cons)
    g1 = np.frombuffer(_fp(bls.G1.gen[0]) + _fp(bls.G1.gen[1]), dtype=np.uint64)
    g2 = np.frombuffer(b"".join(_fp(c) for c in (bls.G2.gen[0][0], bls.G2.gen[0][1], bls.G2.gen[1][0], bls.G2.gen[1][1])), dtype=np.uint64)
    params = pg.Parameters.generate(worker, r1cs, g1, g2, *[rnd.randrange(1, Q) for _ in range(5)])
    proofs, images = [], []
    for _ in range(4):
        xl, xr = rnd.randrange(Q), rnd.randrange(Q)
        images.append(circuits.mimc_hash(xl, xr, cons))
        proofs.append(pg.create_random_proof(circuits.mimc_circuit(xl, xr, cons), params, rng=rnd, r1cs=r1cs))
    return params, proofs, images


def rerandomised(worker, proofs, images, n):
    """n proof records (384 B each, bytes) and their inputs: (A / theta, B theta, C) of the four proofs"""
    lib = _lib.load()
    rnd = random.Random(n)
    recs, ins = [], []
    for k, (base, im) in enumerate(zip(proofs, images)):
        m = n // 4 + (1 if k < n % 4 else 0)
        if not m:
            continue
        th = [rnd.randrange(1, Q) for _ in range(m)]
        out = []
        for group, pt, vals in ((1, base.a, [pow(t, -1, Q) for t in th]), (2, base.b, th)):
            w = 12 if group == 1 else 24
            s = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()
            ds, do = worker.alloc(m * 32), worker.alloc(m * 8 * w)
            worker.upload(ds, s)
            assert lib.bh_fixed_base_mul_dev(worker.ctx, group, np.ascontiguousarray(pt).ctypes.data_as(ctypes.c_void_p), ds, m, 0,
                                             do, None) == 0
            worker.synchronize()
            h = np.zeros((m, w), dtype=np.uint64)
            worker.download(h, do)
            worker.free(ds)
            worker.free(do)
            out.append(h)
        c = np.tile(base.c, (m, 1))
        recs.append(np.concatenate([out[0], out[1], c], axis=1))
        ins += [im] * m
    return np.ascontiguousarray(np.concatenate(recs)), ins


STAGES = (("g2_lines", ("g2_lines_kernel",)), ("z_times_a_and_checks", ("proof_prep_kernel",)), ("miller_loops", ("miller_kernel",)),
          ("product_tree", ("f12_fold_kernel",)), ("final_exponentiation", ("fe_easy_kernel", "fe_mul_op_kernel", "fe_exp_x_kernel",
                                                                            "fe_cyc_sqr_kernel", "fe_finish_kernel")),
          ("fr_column_sums", ("fr_colsum_kernel", "fr_colsum_finish_kernel")), ("alpha_times_acc_y", ("g1_mul_one_kernel",)))


def merge(bench_path, csv_path):
    """the stage times of a --quick run under `rocprofv3 --kernel-trace --stats`: 5 verify_proof calls (one final
    exponentiation each) and two 2^14-proof batches (1 and 16 inputs).  A batch's lines / prep / Miller launch is the
    longest launch of its kernel; the final exponentiation is the mean over the 7 checks."""
    import csv

    res = json.loads(open(bench_path).read().strip().splitlines()[-1])
    rows = list(csv.DictReader(open(csv_path)))
    by = {}
    for r in rows:
        name = r["Name"].split("(")[0].replace("void ", "").replace("bh::", "").strip()
        by[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                    "max_ms": float(r["MaxNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6}
    stages = {}
    for stage, names in STAGES:
        got = [by[n] for n in names if n in by]
        stages[stage] = {"calls": sum(g["calls"] for g in got), "total_ms": sum(g["total_ms"] for g in got),
                         "longest_launch_ms": max((g["max_ms"] for g in got), default=0.0)}
    msm = [v for k, v in by.items() if k.startswith("msm_")]
    stages["multiexps"] = {"calls": sum(g["calls"] for g in msm), "total_ms": sum(g["total_ms"] for g in msm)}
    res["kernel_trace_quick"] = stages
    fe = stages["final_exponentiation"]["total_ms"] / 7
    res["final_exponentiation_ms"] = fe
    miller_s = stages["miller_loops"]["longest_launch_ms"] / 1e3
    rate = (1 << 14) * MILLER / miller_s
    res["miller_2p14"] = {"ms": miller_s * 1e3, "fp_products_per_s": rate, "share_of_ceiling": rate / CEILING}
    print(json.dumps(res))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--merge":
        return merge(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one batch of 2^14 proofs and 5 single verifications (profiling runs)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    w = bellman_amd.Worker(0)
    params, proofs, images = fixture(w)
    pvk = verifier.prepare_verifying_key(params)
    res = {"tool": "bench_verify", "library": _lib.library_identity(), "cpu_baseline": None,
           "fp_products_per_proof": dict(PER_PROOF, total=sum(PER_PROOF.values())), "ceiling_fp_products_per_s": CEILING}
    # verify_proof latency
    raw = np.concatenate([proofs[0].a, proofs[0].b, proofs[0].c]).astype(np.uint64)
    inp = verifier._fr_bytes([images[0]])
    lat = []
    for i in range(5 if a.quick else 50):
        t0 = time.perf_counter()
        rc = lib.bh_groth16_verify(pvk._h, raw.ctypes.data_as(ctypes.c_void_p), inp, 1, 0)
        lat.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, rc
    res["verify_proof_ms"] = {"median": statistics.median(lat[1:]), "min": min(lat[1:])}
    # batches
    sizes = [1 << 14] if a.quick else [1 << 10, 1 << 14, 1 << 16]
    recs, ins = rerandomised(w, proofs, images, max(sizes))
    rnd = random.Random(1)
    z = np.frombuffer(b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(max(sizes))), dtype=np.uint8).copy()
    _, ic = params.vk_ext()
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, _ = params.vk_ext()
    # a 16-input key: 15 further ic points (copies of ic_1); inputs are random
    extra = np.tile(ic[1], (15, 1))
    pvk16 = verifier.PreparedVerifyingKey.from_elements(w, alpha_g1, beta_g2, gamma_g2, delta_g2, np.concatenate([ic, extra]))
    ins16 = np.frombuffer(b"".join(rnd.randrange(Q).to_bytes(32, "little") for _ in range(16 * max(sizes))), dtype=np.uint8).copy()
    ins1 = np.frombuffer(verifier._fr_bytes(ins), dtype=np.uint8).copy()
    batches = {}
    for n in sizes:
        for n_in, key, inputs, want in ((1, pvk, ins1, 0), (16, pvk16, ins16, 9)):
            ts = []
            for _ in range(1 if a.quick else a.reps):
                t0 = time.perf_counter()
                rc = lib.bh_groth16_batch_verify(key._h, recs.ctypes.data_as(ctypes.c_void_p), n,
                                                 inputs.ctypes.data_as(ctypes.c_void_p), n_in, 0, z.ctypes.data_as(ctypes.c_void_p))
                ts.append(time.perf_counter() - t0)
                assert rc == want, (n, n_in, rc)
            t = statistics.median(ts)
            batches["n%d_inputs%d" % (n, n_in)] = {"seconds": t, "proofs_per_s": n / t}
    res["batch"] = batches
    res["target_proofs_per_s_2p16"] = 0.9e6
    pvk16.release()
    pvk.release()
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
