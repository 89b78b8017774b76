"""Proofs of several verifying keys in one call (bh_groth16_verify_each_keys, bh_groth16_batch_verify_keys, csrc/pairing.hip)
against the only way the library had before them: one call per key over the proofs split by key on the host.

Writes profiles/verify_keys_bench.json.  Method of tools/bench_verify_each.py: host wall time of synchronous calls (each
ends in a stream synchronisation), here the MINIMUM over --reps (5) repetitions, the two sides of a comparison interleaved
repetition by repetition in one process after one warm-up call per shape.  Fixture as there: MiMC-322 proofs re-randomised
into as many valid proofs as a call needs; the keys with 7 and 5 inputs are the MiMC key with further ic points and random
inputs, so their proofs fail the pairing check after exactly the work of valid ones (verdicts 9; the batch returns 9).

  K = 3 keys (7, 5 and 1 inputs), 2^10, 2^14 and 2^16 proofs split evenly, rows strictly interleaved in the caller's order:
      one bh_groth16_verify_each_keys call against the sum of three bh_groth16_verify_each calls;
      one bh_groth16_batch_verify_keys call against the sum of three bh_groth16_batch_verify calls.
  K = 1 (the 1-input key): the set call against the single-key entry point - what the grouping and the key lookup cost.
Only the grouped row layout was built (the host sorts a chunk's rows by key), so there is no second layout to compare.

The condition: a one-call form is not slower than the per-key calls it replaces, at any measured size, beyond the 6 % by
which boxes of the pool differ (README), applied within this run.  Exits 1 when it is not met.

  python tools/bench_verify_keys.py [--reps K] [--sizes 1024,16384,65536] [--out FILE]"""

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
OUT = os.path.join(ROOT, "profiles", "verify_keys_bench.json")
MARGIN = 1.06
N_INPUTS = (7, 5, 1)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def compare(one_call, per_key_calls, reps):
    """min over reps of the one call and of the SUM of the per-key calls, interleaved; one warm-up each"""
    one_call()
    for f in per_key_calls:
        f()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(one_call))
        b.append(sum(timed(f) for f in per_key_calls))
    return min(a), min(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,16384,65536")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    import bench_verify as bv
    import bellman_amd
    from bellman_amd import _lib, verifier

    lib = _lib.load()
    w = bellman_amd.Worker(0)
    params, proofs, images = bv.fixture(w)
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    pvks = [verifier.PreparedVerifyingKey.from_elements(w, alpha_g1, beta_g2, gamma_g2, delta_g2,
                                                        np.concatenate([ic, np.tile(ic[1], (n_in - 1, 1))])) for n_in in N_INPUTS]
    set3 = verifier.KeySet(pvks)
    set1 = verifier.KeySet(pvks[2:])
    rnd = random.Random(1)
    recs, ins = bv.rerandomised(w, proofs, images, max(sizes))
    res = {"tool": "bench_verify_keys", "library": _lib.library_identity(), "reps": args.reps, "keys_inputs": list(N_INPUTS),
           "row_layout": "grouped by key on the host (the only layout built)",
           "what": "wall seconds of synchronous calls, min over reps, one call against the sum of the per-key calls, interleaved",
           "margin": MARGIN, "sizes": {}}
    met = True
    for n in sizes:
        key_of = np.arange(n, dtype=np.uint32) % 3
        rows_of = [np.nonzero(key_of == k)[0] for k in range(3)]
        # inputs: the true image for the 1-input key, random scalars for the others
        per_row = [verifier._fr_bytes([ins[j]]) if key_of[j] == 2 else
                   b"".join(rnd.randrange(verifier.Q).to_bytes(32, "little") for _ in range(N_INPUTS[key_of[j]])) for j in range(n)]
        ragged = np.frombuffer(b"".join(per_row), dtype=np.uint8).copy()
        total = len(ragged) // 32
        z = np.frombuffer(b"".join(rnd.randrange(1, verifier.Q).to_bytes(32, "little") for _ in range(n)), dtype=np.uint8).copy().reshape(n, 32)
        sub = []
        for k in range(3):
            r = rows_of[k]
            sub.append((np.ascontiguousarray(recs[r]), np.frombuffer(b"".join(per_row[j] for j in r), dtype=np.uint8).copy(),
                        np.ascontiguousarray(z[r]), len(r)))
        verdicts = np.zeros(n, dtype=np.int32)
        n_bad = ctypes.c_size_t(0)
        want_bad = len(rows_of[0]) + len(rows_of[1])

        def each_one():
            assert lib.bh_groth16_verify_each_keys(set3._h, _p(key_of), _p(recs), n, _p(ragged), total, 0, _p(verdicts),
                                                   ctypes.byref(n_bad)) == 0 and n_bad.value == want_bad

        def each_key(k):
            rk, ik, _, m = sub[k]
            v = np.zeros(m, dtype=np.int32)

            def f():
                assert lib.bh_groth16_verify_each(pvks[k]._h, _p(rk), m, _p(ik), N_INPUTS[k], 0, _p(v), None) == 0
            return f

        def batch_one():
            assert lib.bh_groth16_batch_verify_keys(set3._h, _p(key_of), _p(recs), n, _p(ragged), total, 0, _p(z)) == 9

        def batch_key(k):
            rk, ik, zk, m = sub[k]

            def f():
                assert lib.bh_groth16_batch_verify(pvks[k]._h, _p(rk), m, _p(ik), N_INPUTS[k], 0, _p(zk)) == (0 if k == 2 else 9)
            return f

        r1, i1, z1, m1 = sub[2]
        zeros = np.zeros(m1, dtype=np.uint32)
        v1 = np.zeros(m1, dtype=np.int32)

        def each_set1():
            assert lib.bh_groth16_verify_each_keys(set1._h, _p(zeros), _p(r1), m1, _p(i1), m1, 0, _p(v1), None) == 0

        def batch_set1():
            assert lib.bh_groth16_batch_verify_keys(set1._h, _p(zeros), _p(r1), m1, _p(i1), m1, 0, _p(z1)) == 0

        entry = {}
        for name, one, per_key in (("verify_each_3_keys", each_one, [each_key(k) for k in range(3)]),
                                   ("batch_verify_3_keys", batch_one, [batch_key(k) for k in range(3)]),
                                   ("verify_each_1_key_n%d" % m1, each_set1, [each_key(2)]),
                                   ("batch_verify_1_key_n%d" % m1, batch_set1, [batch_key(2)])):
            a, b = compare(one, per_key, args.reps)
            ok = a <= MARGIN * b
            met = met and ok
            entry[name] = {"one_call_s": a, "per_key_calls_s": b, "per_key_over_one_call": b / a, "not_slower_within_margin": ok}
        res["sizes"]["n%d" % n] = entry
    res["condition"] = {"what": "no one-call form slower than the per-key calls it replaces by more than the margin, at any size",
                        "met": met}
    set1.release()
    set3.release()
    for p in pvks:
        p.release()
    w.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
