"""Proof::read on the device (csrc/point_read.hip): bh_proofs_read alone, batch verification from the bytes Proof::write
emits against batch verification of the same proofs already decoded, and THE GATE: reading the proofs' 2 n G1 + n G2 points
compressed and checked (bh_bases_read_compressed: square root + endomorphism subgroup test) against reading the same
points uncompressed and checked (bh_bases_read_uncompressed: the [q] P kernel), alternating in one process.

Wall time of the synchronous call (each ends with a stream synchronise), one warm-up call, medians of --reps.  Fixture and
re-randomised proofs as tools/bench_verify.py.  Automatic window tables at registration are switched off for the run
(BELLMAN_HIP_TABLE_MAX_LOG2=0): both readers would build the same table after reading, which is not what is compared.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--quick).

Usage: python tools/bench_proof_read.py [--quick] [--reps K]
       python tools/bench_proof_read.py --merge BENCH_JSON KERNEL_STATS_CSV"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ.setdefault("BELLMAN_HIP_TABLE_MAX_LOG2", "0")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bellman_amd  # noqa: E402
import bench_verify as bv  # noqa: E402
from bellman_amd import _lib, verifier  # noqa: E402

P, Q = bv.P, bv.Q
CEILING = bv.CEILING


# ---- Fp products per point, counted from the formulas (csrc/point_read.cuh, point_read.hip, ec.cuh) -------------------------
def pow_schedule_products():
    """a^((p-3)/4) by the sliding window of point_read.cuh (windows of at most 3 bits over a, a^3, a^5, a^7):
    (squarings, products) including the four powers"""
    e = (P - 3) // 4
    bits = bin(e)[2:]
    i, sq, mul, lead = 0, 1, 3, True      # a^2, then a^3, a^5, a^7
    while i < len(bits):
        if bits[i] == "0":
            sq += 1
            i += 1
            continue
        ln = min(3, len(bits) - i)
        while bits[i + ln - 1] == "0":
            ln -= 1
        if not lead:
            sq += ln
            mul += 1
        lead = False
        i += ln
    return sq, mul


SQ, MUL = pow_schedule_products()
FP_ROOT = SQ + MUL + 2                                   # + w a and the test r^2 = a
G1_DBL, G1_MADD, G1_ADD = 9, 10, 14                      # xyzz_dbl 6M + 3S, xyzz_madd 8M + 2S, xyzz_add 12M + 2S
G2_DBL, G2_MADD = 6 * 3 + 3 * 2, 8 * 3 + 2 * 2           # the same over Fp2: a product is 3 Fp products, a square 2
Z_BITS, Z_ADDS = 63, 5                                   # |z| = 0xd201000000010000: 63 doublings, 5 additions
QW = bin(Q).count("1") - 1
PRODUCTS = {
    "g1_read": 2 + 2 + FP_ROOT + 1 + Z_BITS * G1_DBL * 2 + Z_ADDS * (G1_MADD + G1_ADD) + 3,
    "g2_read": 4 + 5 + 2 + 2 * FP_ROOT + 1 + 2 + Z_BITS * G2_DBL + Z_ADDS * G2_MADD + 12,
    "g1_q_test": 5 + 254 * G1_DBL + QW * G1_MADD,        # point_check_kernel: on-curve + [q] P by double-and-add
    "g2_q_test": 15 + 254 * G2_DBL + QW * G2_MADD,
}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def merge(bench_path, csv_path):
    import csv

    res = json.loads(open(bench_path).read().strip().splitlines()[-1])
    n = res["quick_proofs"]
    kern = {}
    for r in csv.DictReader(open(csv_path)):
        name = r["Name"].replace("void ", "").replace("bh::", "")
        for key, pat, pts, prod in (("g1_read", "read_compressed_kernel<FpOps>", 2 * n, "g1_read"),
                                    ("g2_read", "read_compressed_kernel<Fp2Ops>", n, "g2_read"),
                                    ("g1_q_test", "point_check_kernel<FpOps>", 2 * n, "g1_q_test"),
                                    ("g2_q_test", "point_check_kernel<Fp2Ops>", n, "g2_q_test")):
            if name.startswith(pat):
                ms = float(r["MaxNs"]) / 1e6      # the longest launch: the one over all points of the group
                rate = pts * PRODUCTS[prod] / (ms / 1e3)
                kern[key] = {"calls": int(r["Calls"]), "longest_launch_ms": ms, "points": pts, "fp_products_per_s": rate,
                             "share_of_ceiling": rate / CEILING}
    res["kernel_trace_quick"] = kern
    print(json.dumps(res))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--merge":
        return merge(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^16 proofs only, one repetition (profiling runs)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    w = bellman_amd.Worker(0)
    params, proofs, images = bv.fixture(w)
    pvk = verifier.prepare_verifying_key(params)
    sizes = [1 << 16] if a.quick else [1 << 10, 1 << 14, 1 << 16]
    reps = 1 if a.quick else a.reps
    nmax = max(sizes)
    recs, ins = bv.rerandomised(w, proofs, images, nmax)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    packed = np.zeros((nmax, 192), dtype=np.uint8)
    for i in range(nmax):
        lib.bh_proof_write(ctypes.c_void_p(recs.ctypes.data + 384 * i), ctypes.c_void_p(packed.ctypes.data + 192 * i))
    import random

    rnd = random.Random(1)
    z = np.frombuffer(b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(nmax)), dtype=np.uint8).copy()
    ins1 = np.frombuffer(verifier._fr_bytes(ins), dtype=np.uint8).copy()
    res = {"tool": "bench_proof_read", "library": _lib.library_identity(), "reps": reps, "fp_products_per_point": PRODUCTS,
           "ceiling_fp_products_per_s": CEILING, "quick_proofs": nmax}
    out = np.zeros((nmax, 48), dtype=np.uint64)
    status = np.zeros(nmax, dtype=np.uint32)
    res["proofs_read"], res["batch_verify"] = {}, {}
    for n in sizes:
        def read():
            assert lib.bh_proofs_read(w.ctx, p(packed), n, p(out), p(status), None) == 0

        t = timed(read, reps)
        assert (out[:n] == recs[:n]).all() and not status[:n].any()
        res["proofs_read"]["n%d" % n] = {"ms": t * 1e3, "proofs_per_s": n / t}

        def from_bytes():
            assert lib.bh_groth16_batch_verify_compressed(pvk._h, p(packed), n, p(ins1), 1, 0, p(z), None) == 0

        def affine():
            assert lib.bh_groth16_batch_verify(pvk._h, p(recs), n, p(ins1), 1, 0, p(z)) == 0

        tb, ta = [], []
        from_bytes()
        affine()
        for _ in range(reps):   # alternating
            for fn, ts in ((from_bytes, tb), (affine, ta)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        tb, ta = statistics.median(tb), statistics.median(ta)
        res["batch_verify"]["n%d" % n] = {"compressed_ms": tb * 1e3, "compressed_proofs_per_s": n / tb, "affine_ms": ta * 1e3,
                                          "affine_proofs_per_s": n / ta}
    # ---- the gate: the 2 n G1 + n G2 points of the proofs, compressed + checked against uncompressed + checked -----------
    n = nmax
    gate = {}
    for group, name in ((1, "g1"), (2, "g2")):
        if group == 1:
            comp = np.ascontiguousarray(np.concatenate([packed[:n, :48], packed[:n, 144:]]))
            aff = np.ascontiguousarray(np.concatenate([recs[:n, :12], recs[:n, 36:]]))
        else:
            comp = np.ascontiguousarray(packed[:n, 48:144])
            aff = np.ascontiguousarray(recs[:n, 12:36])
        m = aff.shape[0]
        hb = bellman_amd.Bases(w, group, aff)
        unc = np.zeros(m * aff.shape[1] * 8, dtype=np.uint8)
        assert lib.bh_bases_write_uncompressed(w.ctx, hb._h, 0, m, p(unc)) == 0
        del hb

        def rd(fn, buf):
            h = ctypes.c_void_p()
            assert fn(w.ctx, group, p(buf), m, 1 | 2, ctypes.byref(h), None) == 0
            return h

        # both readers give the same records
        h1, h2 = rd(lib.bh_bases_read_compressed, comp), rd(lib.bh_bases_read_uncompressed, unc)
        o1, o2 = np.zeros_like(aff), np.zeros_like(aff)
        assert lib.bh_bases_download(w.ctx, h1, 0, m, p(o1)) == 0 and lib.bh_bases_download(w.ctx, h2, 0, m, p(o2)) == 0
        assert (o1 == aff).all() and (o2 == aff).all()
        lib.bh_bases_release(w.ctx, h1)
        lib.bh_bases_release(w.ctx, h2)
        tc, tu = [], []
        for _ in range(reps):   # alternating
            for fn, buf, ts in ((lib.bh_bases_read_compressed, comp, tc), (lib.bh_bases_read_uncompressed, unc, tu)):
                t0 = time.perf_counter()
                h = rd(fn, buf)
                ts.append(time.perf_counter() - t0)
                lib.bh_bases_release(w.ctx, h)
        tc, tu = statistics.median(tc), statistics.median(tu)
        gate[name] = {"points": m, "compressed_checked_ms": tc * 1e3, "uncompressed_checked_ms": tu * 1e3,
                      "ratio": tc / tu, "passes": bool(tc <= tu)}
    res["gate"] = gate
    pvk.release()
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
