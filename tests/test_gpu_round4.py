"""GPU parity of what round 4 changed on the hot path (run with `pytest -m gpu` on a MI355X).  The kernels themselves
(fused last line of the mixed addition, G2 accumulation on lane pairs, lazily reduced FFT butterflies, one-level FFT
tables) sit under every multiexp / FFT test of the suite; here are the cases that need a special set-up:

  * the FFT's two-level tables (what sizes above 2^24 and a failed table allocation use) at sizes that take the
    one-level tables by default (src/domain.rs:81-125);
  * the G1 window table at a 128-byte record stride (vectors of 2^19 ... 2^22 points) under every variant of the bucket
    accumulation and against the classic plan over the same vector (src/multiexp.rs:210-332).
Integer work: every limb equal, no tolerances."""

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_groth16 import worker  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SNIPPET = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
import bellman_amd
from bellman_amd import _lib
from oracle import cref
lib = _lib.load()
w = bellman_amd.Worker(0)
for log_n in (12, 13, 17, 22):
    n = 1 << log_n
    data = cref.random_fr(n, 4400 + log_n)
    for mode in (0, 1, 2, 3):
        d = bellman_amd.EvaluationDomain.from_coeffs(w, data)
        [d.fft, d.ifft, d.coset_fft, d.icoset_fft][mode]()
        assert np.array_equal(d.into_coeffs(), cref.fft(data, mode)), (log_n, mode)
print("ok", flush=True)
"""


@pytest.mark.parametrize("one_level", ["0", "1"])
def test_fft_with_two_level_and_one_level_tables(one_level):
    """BELLMAN_HIP_FFT_ONE_LEVEL=0 forces the hi x lo tables (two products per twiddle / coset factor, the 1/n as a
    separate product) at sizes that by default read one-level tables in element order (one product, 1/n folded into the
    inverse twiddles): all four transforms == the restated best_fft at 2^12, 2^13, 2^17, 2^22, either way.  (The switch is
    read once per process, hence the subprocess.)"""
    env = dict(os.environ, BELLMAN_HIP_FFT_ONE_LEVEL=one_level)
    r = subprocess.run([sys.executable, "-c", _SNIPPET % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_large_host_scalar_multiexp_error_semantics(worker):
    """bh_msm_async with 2^19 + 777 HOST scalars (what a Rust host with only multiexp.rs patched issues per multiexp):
    result and error semantics of src/multiexp.rs:210-332 at a size where the full pipeline runs - == the oracle with a
    density map and skip; running out of bases near the end, or a quarter of the way in; an identity base early or late
    with a full-size scalar (top window: wins over a later EOF) or a small one (the EOF wins), or under a zero scalar
    (never seen).  (Written for the round-4 experiment that issued such a multiexp as two halves so that the second
    half's upload would overlap the first half's kernels: no gain - each half pays the latency-bound stages and a host
    tail of its own, profiles/archive/r4_call8.txt - removed; the cases stay.)"""
    import bellman_amd
    from bellman_amd import UnexpectedEof, UnexpectedIdentity
    from oracle import cref

    n = (1 << 19) + 777
    rnd = np.random.default_rng(41)
    bases = cref.gen_bases(1, n + 100, a=3, b=5)
    sc = cref.random_fr(n, 4100)
    dens = rnd.random(n) < 0.6
    dm = bellman_amd.DensityTracker(dens)
    hb = bellman_amd.Bases(worker, 1, bases)

    def run(hbases, scalars, density, skip, host_bases):
        rc, want = cref.multiexp(1, host_bases, skip, None if density is None else cref.density_bitmap(density), scalars,
                                 threads=cref.lib().orc_max_threads())
        d = bellman_amd.FullDensity() if density is None else bellman_amd.DensityTracker(density)
        try:
            got = bellman_amd.multiexp(worker, hbases, d, scalars, skip=skip).wait()
            assert rc == 0 and np.array_equal(got, want)
            out = 0
        except UnexpectedIdentity:
            out = 1
        except UnexpectedEof:
            out = 2
        assert out == rc, (out, rc)
        return rc

    assert run(hb, sc, None, 0, bases) == 0
    assert run(hb, sc, dens, 37, bases) == 0
    del dm
    short = bases[: n - 5]                                   # the upper half runs out of bases
    hs = bellman_amd.Bases(worker, 1, short)
    assert run(hs, sc, None, 0, short) == 2
    tiny = bases[: n // 4]                                   # ... the lower half already does
    ht = bellman_amd.Bases(worker, 1, tiny)
    assert run(ht, sc, None, 0, tiny) == 2
    for pos in (1000, n - 2000):                             # an identity in the lower / the upper half
        b2 = bases.copy()
        b2[pos] = 0
        s2 = sc.copy()
        s2[pos] = cref.ints_to_arr([cref.Q - 1], 4)[0]       # non-zero top window
        h2 = bellman_amd.Bases(worker, 1, b2)
        assert run(h2, s2, None, 0, b2) == 1
        h2s = bellman_amd.Bases(worker, 1, b2[: n - 5])
        assert run(h2s, s2, None, 0, b2[: n - 5]) == 1       # ... wins over the EOF that comes later
        s2[pos] = cref.ints_to_arr([5], 4)[0]                # small scalar: zero top digit, the EOF wins
        assert run(h2s, s2, None, 0, b2[: n - 5]) == 2
        s2[pos] = 0                                          # zero scalar: the identity is skipped unseen
        assert run(h2, s2, None, 0, b2) == 0
        h2.release()
        h2s.release()
    for h in (hb, hs, ht):
        h.release()


def test_g1_window_table_at_128_byte_stride(worker):
    """A G1 vector of 2^19 points with its window table built at a 128-byte record stride (api_bases.hip
    bh_bases::table_stride; 16-bit and 20-bit rows): the multiexp over it == the classic 16-window plan over the dense
    vector == [sum s_i t_i]G, with full density, with a density map + skip, with a forced chunk length and with the
    LDS-accumulator variant of the kernel (every variant takes the record stride).  Then the error semantics of
    src/multiexp.rs:55-80,295-300 on that path - the error-resolution kernel reads row 0 of the table at its stride: an
    identity base under a full-size / small / zero scalar, running out of bases, and both at once == what the classic plan
    reports for the same inputs (itself == the oracle in test_large_host_scalar_multiexp_error_semantics).  (Until round 6
    such tables were built on request only - bh_bases_precompute, BELLMAN_HIP_TABLE_MAX_LOG2_G1; a registered vector of up
    to 2^22 points now gets its 20-bit table automatically.)"""
    import bellman_amd
    import importlib
    from oracle import cref
    from tests.test_gpu_scale import _device_bases, _splitmix

    mx = importlib.import_module("bellman_amd.multiexp")
    n = 1 << 19
    t = _splitmix(n, 4190)
    bases, _host, gen = _device_bases(worker, 1, t, table=False)   # a wrapped device vector: no table yet
    sc = _splitmix(n, 4191)
    rnd = np.random.default_rng(419)
    m, skip = n - 4321, 5
    bits = rnd.random(m) < 0.5
    dt = bellman_amd.DensityTracker()
    dt.bv = bits
    cases = [("full", dict(density_map=bellman_amd.FullDensity(), exponents=sc)),
             ("short + skip", dict(density_map=bellman_amd.FullDensity(), exponents=sc[: n - 12345], skip=777)),
             ("density + skip", dict(density_map=dt, exponents=sc[:m], skip=skip))]
    want = {name: bellman_amd.multiexp(worker, bases, flags=mx.NO_TABLE, **kw).wait() for name, kw in cases}
    assert np.array_equal(want["full"], cref.point_mul(1, gen, cref.fr_dot(sc, t)))
    assert np.array_equal(want["density + skip"], cref.point_mul(1, gen, cref.fr_dot(sc[:m][bits], t[skip:skip + int(bits.sum())])))
    for c in (16, 20):
        bases.precompute(c)
        c_used, rows, nbytes = bases.table_info()
        assert c_used == c and rows == (256 + c - 1) // c and nbytes == rows * n * 128   # one cache line per record
        for name, kw in cases:
            for flags, chunk in ((0, 0), (mx.ACC_LDS, 0), (0, 64), (mx.NO_SMALL_PATH, 0)):
                got = bellman_amd.multiexp(worker, bases, flags=flags, chunk=chunk, **kw).wait()
                assert np.array_equal(got, want[name]), (c, name, flags, chunk)
    bases.release()

    from bellman_amd import UnexpectedEof, UnexpectedIdentity

    def outcome(hb, scalars, flags):
        try:
            return 0, bellman_amd.multiexp(worker, hb, bellman_amd.FullDensity(), scalars, flags=flags).wait()
        except UnexpectedIdentity:
            return 1, None
        except UnexpectedEof:
            return 2, None

    # one scalar more than there are bases = the reference's UnexpectedEof on the last term; the vectors stay at 2^19
    # records so that their tables are the ones at the 128-byte stride
    full = np.vstack([sc, sc[:1]])
    full[:, 3] |= np.uint64(1 << 60)          # a non-zero top-window digit everywhere
    small = full.copy()
    small[17] = cref.ints_to_arr([5], 4)[0]   # the identity base is then met in window 0 only
    zero = full.copy()
    zero[17] = 0
    b2 = _host.copy()
    b2[17] = 0                                # identity record
    expect = {}
    for tag, bs, count in (("identity", b2, n), ("identity, one base short", b2, n + 1), ("one base short", _host, n + 1)):
        hb = bellman_amd.Bases(worker, 1, bs)
        assert hb.table_info()[:2] == (20, 13)     # [r6] the automatic 20-bit table of a 2^19-point vector; NO_TABLE declines it
        for sname, scal in (("full", full), ("small", small), ("zero", zero)):
            expect[tag, sname] = outcome(hb, scal[:count], mx.NO_TABLE)
        hb.precompute(16)
        assert hb.table_info()[2] == 16 * n * 128
        for sname, scal in (("full", full), ("small", small), ("zero", zero)):
            rc, val = outcome(hb, scal[:count], 0)
            assert rc == expect[tag, sname][0], (tag, sname, rc, expect[tag, sname][0])
            if rc == 0:
                assert np.array_equal(val, expect[tag, sname][1]), (tag, sname)
        hb.release()
    assert expect["identity", "full"][0] == 1 and expect["identity", "zero"][0] == 0 and expect["one base short", "full"][0] == 2
    assert expect["identity, one base short", "full"][0] == 1 and expect["identity, one base short", "small"][0] == 2
