"""The word-program witness generator (bh_word_witness_generate_dev) against the witness solver (bh_r1cs_solve_many_dev) on the
same SHA-256 preimage circuits, and against uploading as many bytes of host-made witnesses.

Method (that of tools/bench_r1cs_solve.py): host wall time from the issue of the call to a final stream synchronisation, min
of REPS repetitions after one warm-up round, the variants and the values of k interleaved in one process.
  word     the external words (the messages) are on the device; bh_word_witness_generate_dev writes every variable
  solver   buffers zeroed, ONE and the message bits uploaded per witness (not timed); bh_r1cs_solve_many_dev with shape.supplied /
           shape.hints completes them
  upload   bh_dev_upload of k x (inputs + aux) x 32 bytes from one pageable host array: what a caller pays who makes the
           witnesses on the host (the synthesis itself is not in this figure)
After the timed runs the first witnesses of the word path are compared byte for byte with host synthesis and
bh_r1cs_check_many_dev must find every one of the k satisfied, for both paths.
Shapes: Sha256Preimage(55) (one block) and (64) (two blocks); k = 16, 256, 4096 (--ks), k is lowered to what fits --max-bytes.
No speed-up is asserted: the rows say what came out.

Usage: python tools/bench_word_witness.py [--out profiles/word_witness_bench.json] [--reps 5] [--ks 16,256,4096]"""
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

SATISFIED = 0xFFFFFFFF
CHECKED = 3   # witnesses compared with the host synthesis


class Shape:
    def __init__(self, worker, lib, circuit, shape, capture_ms, kmax, rnd):
        from bellman_amd import gadgets as g
        from bellman_amd import groth16 as pg

        n_bytes = circuit.n_bytes
        self.worker, self.lib, self.name, self.kmax = worker, lib, "sha256-preimage-%d" % n_bytes, kmax
        self.circuit, self.shape, self.capture_ms = circuit, shape, capture_ms
        c = circuit
        self.r1cs = shape.r1cs(worker)
        t0 = time.perf_counter()
        self.gen = shape.witness_generator(worker)
        self.create_ms = (time.perf_counter() - t0) * 1e3
        self.solver = shape.solver(self.r1cs)
        self.n_in, self.n_aux = shape.num_inputs, shape.num_aux
        self.in_stride, self.aux_stride = self.n_in * 32, self.n_aux * 32
        self.msgs = [bytes(rnd.getrandbits(8) for _ in range(n_bytes)) for _ in range(kmax)]
        self.ext = c.ext_from_messages(self.msgs)
        self.d_ext = worker.alloc(max(self.ext.nbytes, 32))
        worker.upload(self.d_ext, self.ext)
        self.d_in, self.d_aux = worker.alloc(kmax * self.in_stride + 32), worker.alloc(kmax * self.aux_stride + 32)
        self.d_bad = worker.alloc(kmax * 4)
        t0 = time.perf_counter()
        self.expect = [tuple(pg.fr_to_mont_array(v) for v in g.synthesize(c.with_message(m))) for m in self.msgs[:CHECKED]]
        self.host_synthesis_ms = (time.perf_counter() - t0) * 1e3 / CHECKED
        # the message bits of every witness as the solver's supplied values: aux 0 .. 8 n - 1, in order
        sup = [v.idx for v in shape.supplied]
        assert sup == list(range(8 * n_bytes))
        bits = np.unpackbits(np.frombuffer(b"".join(self.msgs), dtype=np.uint8)).reshape(kmax, 8 * n_bytes)
        zero_one = pg.fr_to_mont_array([0, 1])
        self.sup = np.ascontiguousarray(zero_one[bits])   # [kmax, 8 n, 4]
        self.one = pg.fr_to_mont_array([1])
        self.host = None

    def word_ms(self, k):
        t0 = time.perf_counter()
        assert self.lib.bh_word_witness_generate_dev(self.worker.ctx, self.gen._h, self.d_ext, self.ext.shape[1] * 4, self.d_in, self.in_stride,
                                                     self.d_aux, self.aux_stride, k, None) == 0
        self.worker.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def reset(self, k):
        lib, ctx = self.lib, self.worker.ctx
        at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
        assert lib.bh_dev_zero(ctx, self.d_in, k * self.in_stride) == 0 and lib.bh_dev_zero(ctx, self.d_aux, k * self.aux_stride) == 0
        for j in range(k):
            assert lib.bh_dev_upload(ctx, at(self.d_in, j * self.in_stride), self.one.ctypes.data_as(ctypes.c_void_p), 32) == 0
            assert lib.bh_dev_upload(ctx, at(self.d_aux, j * self.aux_stride), self.sup[j].ctypes.data_as(ctypes.c_void_p), self.sup[j].nbytes) == 0
        self.worker.synchronize()

    def solver_ms(self, k):
        self.reset(k)
        t0 = time.perf_counter()
        assert self.lib.bh_r1cs_solve_many_dev(self.worker.ctx, self.solver._h, self.d_in, self.in_stride, self.d_aux, self.aux_stride, k, None) == 0
        self.worker.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def upload_ms(self, k):
        if self.host is None:   # host-made witness bytes: the content does not matter to a copy
            self.host = np.full(self.kmax * (self.n_in + self.n_aux) * 4, 1, dtype=np.uint64)
        n_in, n_aux = k * self.n_in * 4, k * self.n_aux * 4
        t0 = time.perf_counter()
        self.worker.upload(self.d_in, self.host[:n_in])
        self.worker.upload(self.d_aux, self.host[n_in:n_in + n_aux])
        self.worker.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def verify(self, k, compare):
        at = lambda dev, off: ctypes.c_void_p(dev.value + off)  # noqa: E731
        if compare:
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

    def close(self):
        for d in (self.d_ext, self.d_in, self.d_aux, self.d_bad):
            self.worker.free(d)
        self.gen.release()
        self.solver.release()
        self.r1cs.release()
        self.host = None
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_witness_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="16,256,4096")
    ap.add_argument("--sizes", default="55,64")
    ap.add_argument("--max-bytes", type=int, default=16 << 30, help="device bytes of the witness buffers of one shape")
    args = ap.parse_args()
    import bellman_amd
    from bellman_amd import _lib

    lib = _lib.load()
    worker = bellman_amd.Worker(0)
    rnd = random.Random(2026)
    rows = []
    for n_bytes in [int(x) for x in args.sizes.split(",")]:
        from bellman_amd import gadgets as g

        circuit = g.Sha256Preimage(n_bytes)
        t0 = time.perf_counter()
        shape = g.capture(circuit)
        capture_ms = (time.perf_counter() - t0) * 1e3
        per_witness = (shape.num_inputs + shape.num_aux) * 32
        fit = max(args.max_bytes // per_witness, 1)
        ks = sorted({min(int(x), fit) for x in args.ks.split(",")})   # the largest k that fits where a k does not
        sh = Shape(worker, lib, circuit, shape, capture_ms, max(ks), rnd)
        variants = []
        for k in ks:
            variants += [(("word", k), lambda k=k: sh.word_ms(k)), (("solver", k), lambda k=k: sh.solver_ms(k)),
                         (("upload", k), lambda k=k: sh.upload_ms(k))]
        times = interleaved(variants, args.reps)
        for k in ks:
            sh.solver_ms(k)
            sh.verify(k, False)
            sh.word_ms(k)
            sh.verify(k, True)
            tw, ts, tu = times[("word", k)], times[("solver", k)], times[("upload", k)]
            nbytes = k * per_witness
            row = {"circuit": sh.name, "constraints": sh.shape.num_constraints, "variables": sh.n_in + sh.n_aux, "k": k,
                   "program": {"words": int(sh.shape.n_ext + len(sh.shape.program["instrs"])), "external_words": int(sh.shape.n_ext)},
                   "solver_plan": sh.solver.info, "capture_ms": round(sh.capture_ms, 1), "word_witness_create_ms": round(sh.create_ms, 2),
                   "host_synthesis_ms_per_witness": round(sh.host_synthesis_ms, 1), "witness_bytes": nbytes,
                   "word_ms": tw, "word_min": min(tw), "word_spread": round(max(tw) - min(tw), 4),
                   "word_us_per_witness": round(min(tw) * 1e3 / k, 3), "word_bytes_written_per_s": round(nbytes / (min(tw) * 1e-3)),
                   "solver_ms": ts, "solver_min": min(ts), "solver_spread": round(max(ts) - min(ts), 4),
                   "solver_us_per_witness": round(min(ts) * 1e3 / k, 3),
                   "upload_ms": tu, "upload_min": min(tu), "upload_bytes_per_s": round(nbytes / (min(tu) * 1e-3)),
                   "ratio_solver_over_word": round(min(ts) / min(tw), 3), "ratio_upload_over_word": round(min(tu) / min(tw), 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        sh.close()
    info = worker.info()
    out = {"tool": "tools/bench_word_witness.py",
           "method": "host wall ms from the issue of the call to a final stream sync, min of %d reps after one warm-up round, the three "
                     "variants and the values of k interleaved in one process; the solver's reset (zero, ONE and message bits uploaded) "
                     "and the upload of the external words are not timed" % args.reps,
           "not_measured": "kernel time by rocprofv3, any counter, any share of peak, the host form (bh_word_witness_generate), "
                           "the two kernels apart from each other",
           "device": {"num_cus": info["num_cus"], "hbm_bytes": info["hbm_bytes"]}, "library": _lib.library_identity(), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    worker.close()


if __name__ == "__main__":
    main()
