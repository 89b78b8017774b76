"""EvaluationDomain<Fr, Point<G>> on the device (bh_fft_point_dev and the element-wise point operations of
include/bellman_hip.h, bellman_amd.PointEvaluationDomain): byte-identical affine records against

  * the group-valued restatement of src/domain.rs (tests/point_domain_model.py, group law in the C oracle) at small sizes;
  * linearity at scale: with P_i = [c_i]G the point transform is [scalar transform(c)_j]G, the right side from
    bh_fft_fr_dev and bh_fixed_base_mul_dev (both parity-tested against the oracle elsewhere);
  * the Lagrange basis from powers of tau (generator.rs:299-300 lifted to the group)."""

import ctypes
import os
import random
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import point_domain_model as pdm  # noqa: E402
from tests import scalar_mixes  # noqa: E402

Q = bls.Q
WORDS = {1: 12, 2: 24}
BH_ERR_DEGREE_TOO_LARGE, BH_ERR_INVALID_ARG = 3, -2


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _lib():
    from bellman_amd import _lib as L

    return L.load()


def _mont(ints):
    return cref.fr_to_mont(cref.ints_to_arr([v % Q for v in ints], 4))


def _gen(group):
    return np.ascontiguousarray(cref.g1_generator() if group == 1 else cref.g2_generator())


def _fixed_base(worker, group, scalars_mont):
    """[s_i]G for Montgomery scalars, on the device -> host records"""
    n = scalars_mont.shape[0]
    ds, dout = worker.alloc(n * 32), worker.alloc(n * 8 * WORDS[group])
    worker.upload(ds, np.ascontiguousarray(scalars_mont))
    assert _lib().bh_fixed_base_mul_dev(worker.ctx, group, _p(_gen(group)), ds, n, 1, dout, None) == 0
    out = np.empty((n, WORDS[group]), dtype=np.uint64)
    worker.download(out, dout)
    worker.free(ds)
    worker.free(dout)
    return out


def _scalar_fft(worker, scalars_mont, mode):
    import bellman_amd

    d = bellman_amd.EvaluationDomain.from_coeffs(worker, scalars_mont)
    (d.fft, d.ifft, d.coset_fft, d.icoset_fft)[mode]()
    return d.into_coeffs()


def _point_fft(worker, group, points, mode):
    import bellman_amd

    d = bellman_amd.PointEvaluationDomain.from_coeffs(worker, group, points)
    (d.fft, d.ifft, d.coset_fft, d.icoset_fft)[mode]()
    return d.into_coeffs()


def _random_points(G, n, seed):
    rnd = random.Random(seed)
    return [G.mul(G.gen(), rnd.randrange(1, Q)) for _ in range(n)]


# ---- 1. against the model ------------------------------------------------------------------------------------------
# all four modes up to 2^8 (G1) / 2^6 (G2); the model's group law costs 1-2 ms per scalar multiplication on the host, so
# the largest sizes run the forward transform only (the other modes are covered at scale by linearity below)
MODEL_CASES = [(1, k, m) for k in range(9) for m in range(4)] + [(1, 9, 0), (1, 10, 0)] + \
              [(2, k, m) for k in range(7) for m in range(4)] + [(2, 7, 0), (2, 8, 0)]


@pytest.mark.parametrize("group,log_n,mode", MODEL_CASES)
def test_transform_matches_model(worker, group, log_n, mode):
    G = pdm.PointGroup(group)
    pts = _random_points(G, 1 << log_n, 1000 * group + 10 * log_n + mode)
    if log_n >= 2:
        pts[1] = G.identity()   # identities among the inputs
    d = pdm.PointDomain.from_coeffs(G, pts)
    d.run(mode)
    got = _point_fft(worker, group, G.to_array(pts), mode)
    assert np.array_equal(got, G.to_array(d.coeffs))


@pytest.mark.parametrize("group,log_n", [(1, 0), (1, 3), (1, 7), (2, 0), (2, 5)])
def test_elementwise_ops_match_model(worker, group, log_n):
    import bellman_amd

    G = pdm.PointGroup(group)
    n = 1 << log_n
    rnd = random.Random(group * 100 + log_n)
    pts = _random_points(G, n, 7 + log_n)
    other = _random_points(G, n, 8 + log_n)
    other[0] = pts[0]                                # a - a
    if n > 2:
        other[1] = G.neg(pts[1])                     # a - (-a)
        other[2] = G.identity()                      # a - 0
        pts[3 % n] = G.identity()                    # 0 - b
    scal = [rnd.randrange(Q) for _ in range(n)]
    if n > 2:
        scal[2], scal[1] = 0, 1
    g = rnd.randrange(1, Q)
    d = pdm.PointDomain.from_coeffs(G, pts)
    dev = bellman_amd.PointEvaluationDomain.from_coeffs(worker, group, G.to_array(pts))
    d.distribute_powers(g)
    dev.distribute_powers(worker, _mont([g]))
    assert np.array_equal(dev.as_ref(), G.to_array(d.coeffs))
    d.mul_assign(scal)
    sd = bellman_amd.EvaluationDomain.from_coeffs(worker, _mont(scal))
    dev.mul_assign(worker, sd)
    assert np.array_equal(dev.as_ref(), G.to_array(d.coeffs))
    d.sub_assign(other)
    dev.sub_assign(worker, bellman_amd.PointEvaluationDomain.from_coeffs(worker, group, G.to_array(other)))
    assert np.array_equal(dev.as_ref(), G.to_array(d.coeffs))
    d.divide_by_z_on_coset()
    dev.divide_by_z_on_coset(worker)
    assert np.array_equal(dev.into_coeffs(), G.to_array(d.coeffs))


# ---- 2. linearity at scale -----------------------------------------------------------------------------------------
SCALE_CASES = [(1, 12, m, "uniform") for m in range(4)] + [(1, 12, 0, "bool90"), (1, 12, 1, "small90"), (1, 12, 2, "ones")] + \
              [(1, 16, m, "bool50") for m in range(4)] + [(1, 20, m, "uniform") for m in range(4)] + \
              [(2, 12, m, "uniform") for m in range(4)] + [(2, 12, 0, "bool90")] + \
              [(2, 16, m, "bool50") for m in range(4)] + [(2, 18, 0, "uniform")]


@pytest.mark.parametrize("group,log_n,mode,mix", SCALE_CASES)
def test_linearity_at_scale(worker, group, log_n, mode, mix):
    n = 1 << log_n
    c = cref.fr_to_mont(scalar_mixes.scalars(mix, n, 31 * log_n + mode))
    pts = _fixed_base(worker, group, c)
    want = _fixed_base(worker, group, _scalar_fft(worker, c, mode))
    got = _point_fft(worker, group, pts, mode)
    assert np.array_equal(got, want)


# ---- 3. degenerate inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_degenerate_inputs(worker, group):
    G = pdm.PointGroup(group)
    P = G.mul(G.gen(), 123456789)
    ident = G.identity()
    for log_n in (0, 1, 4, 8):
        n = 1 << log_n
        # all identity: every mode gives the identity
        for mode in range(4):
            assert not _point_fft(worker, group, G.to_array([ident] * n), mode).any()
        # a constant vector: fft gives [n]P at index 0 and the identity elsewhere
        got = _point_fft(worker, group, G.to_array([P] * n), 0)
        assert np.array_equal(got[0], G.to_array([G.mul(P, n)])[0])
        assert not got[1:].any()
        # ... and ifft of [n]P at 0 gives the constant vector back
        back = _point_fft(worker, group, got, 1)
        assert np.array_equal(back, G.to_array([P] * n))
    # one-hot vectors, +-P pairs, boolean-style inputs against the model
    for log_n in (3, 5):
        n = 1 << log_n
        cases = []
        for hot in (0, 1, n - 1):
            v = [ident] * n
            v[hot] = P
            cases.append(v)
        cases.append([P if i % 2 == 0 else G.neg(P) for i in range(n)])
        cases.append([P if (i * 7) % 3 else ident for i in range(n)])
        for v in cases:
            for mode in range(4):
                d = pdm.PointDomain.from_coeffs(G, v)
                d.run(mode)
                assert np.array_equal(_point_fft(worker, group, G.to_array(v), mode), G.to_array(d.coeffs)), mode


@pytest.mark.parametrize("group,length", [(1, 3), (1, 100), (2, 5), (2, 33)])
def test_lengths_not_powers_of_two(worker, group, length):
    """from_coeffs pads with identity records (domain.rs:68)"""
    import bellman_amd

    rnd = np.random.default_rng(length)
    m = 1 << (length - 1).bit_length()
    c = np.zeros((m, 4), dtype=np.uint64)
    c[:length] = cref.fr_to_mont(cref.ints_to_arr([int(x) for x in rnd.integers(1, 1 << 62, length)], 4))
    pts = _fixed_base(worker, group, c)
    d = bellman_amd.PointEvaluationDomain.from_coeffs(worker, group, pts[:length])
    assert len(d) == m
    assert np.array_equal(d.as_ref()[length:], np.zeros((m - length, WORDS[group]), dtype=np.uint64))
    d.coset_fft()
    assert np.array_equal(d.into_coeffs(), _fixed_base(worker, group, _scalar_fft(worker, c, 2)))


# ---- 4. round trips ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,log_n", [(1, 20), (2, 16)])
def test_round_trips(worker, group, log_n):
    import bellman_amd

    n = 1 << log_n
    pts = _fixed_base(worker, group, cref.fr_to_mont(scalar_mixes.scalars("bool50", n, 5)))
    d = bellman_amd.PointEvaluationDomain.from_coeffs(worker, group, pts)
    d.fft()
    d.ifft()
    assert np.array_equal(d.as_ref(), pts)
    d.coset_fft()
    d.icoset_fft()
    assert np.array_equal(d.into_coeffs(), pts)


# ---- 5. Lagrange basis from powers of tau --------------------------------------------------------------------------
@pytest.mark.parametrize("group,log_n", [(1, 16), (2, 14)])
def test_lagrange_basis_from_powers_of_tau(worker, group, log_n):
    """[tau^i]G of a transcript -> ifft -> [L_j(tau)]G, with L_j(tau) from the scalar ifft of the powers (generator.rs:
    299-300)"""
    n = 1 << log_n
    tau = _mont([0x1234_5678_9ABC_DEF0_1357_9BDF_2468_ACE0 * 0x1F2E3D4C5B6A7988 + 3])
    one = _mont([1])
    dpow = worker.alloc(n * 32)
    assert _lib().bh_fr_powers_dev(worker.ctx, dpow, n, _p(tau), _p(one), None) == 0
    worker.synchronize()
    powers = np.empty((n, 4), dtype=np.uint64)
    worker.download(powers, dpow)
    worker.free(dpow)
    transcript = _fixed_base(worker, group, powers)
    lagrange = _fixed_base(worker, group, _scalar_fft(worker, powers, 1))
    assert np.array_equal(_point_fft(worker, group, transcript, 1), lagrange)


# ---- 6. streams and errors -----------------------------------------------------------------------------------------
def test_two_streams_beside_a_multiexp(worker):
    import bellman_amd

    lib = _lib()
    n1, n2 = 1 << 12, 1 << 10
    p1 = _fixed_base(worker, 1, cref.fr_to_mont(scalar_mixes.scalars("uniform", n1, 1)))
    p2 = _fixed_base(worker, 2, cref.fr_to_mont(scalar_mixes.scalars("uniform", n2, 2)))
    want1, want2 = _point_fft(worker, 1, p1, 2), _point_fft(worker, 2, p2, 1)
    bases = cref.gen_bases(1, 1 << 14, a=3, b=5)
    sc = cref.random_fr(1 << 14, 9)
    rc0, want_msm = cref.multiexp(1, bases, 0, None, sc)
    hb = bellman_amd.Bases(worker, 1, bases)
    streams = []
    for _ in range(2):
        s = ctypes.c_void_p()
        assert lib.bh_stream_create(worker.ctx, ctypes.byref(s)) == 0
        streams.append(s)
    d1, d2 = worker.alloc(p1.nbytes), worker.alloc(p2.nbytes)
    worker.upload(d1, p1)
    worker.upload(d2, p2)
    rcs = [None, None]

    def run(k, group, dev, log_n, mode):
        rcs[k] = lib.bh_fft_point_dev(worker.ctx, group, dev, log_n, mode, streams[k])

    ts = [threading.Thread(target=run, args=(0, 1, d1, 12, 2)), threading.Thread(target=run, args=(1, 2, d2, 10, 1))]
    for t in ts:
        t.start()
    got_msm = bellman_amd.multiexp(worker, hb, bellman_amd.FullDensity(), sc).wait()
    for t in ts:
        t.join()
    assert rcs == [0, 0]
    g1, g2 = np.empty_like(p1), np.empty_like(p2)
    worker.download(g1, d1)
    worker.download(g2, d2)
    worker.free(d1)
    worker.free(d2)
    for s in streams:
        assert lib.bh_stream_destroy(worker.ctx, s) == 0
    assert rc0 == 0 and np.array_equal(got_msm, want_msm)
    assert np.array_equal(g1, want1) and np.array_equal(g2, want2)


def test_errors(worker):
    import bellman_amd

    lib = _lib()
    d = worker.alloc(4 * 96)
    worker.upload(d, np.zeros((4, 12), dtype=np.uint64))
    g = _mont([5])
    assert lib.bh_fft_point_dev(worker.ctx, 3, d, 2, 0, None) == BH_ERR_INVALID_ARG
    assert lib.bh_fft_point_dev(worker.ctx, 0, d, 2, 0, None) == BH_ERR_INVALID_ARG
    assert lib.bh_fft_point_dev(worker.ctx, 1, d, 2, 4, None) == BH_ERR_INVALID_ARG
    assert lib.bh_fft_point_dev(worker.ctx, 1, d, 2, -1, None) == BH_ERR_INVALID_ARG
    assert lib.bh_fft_point_dev(worker.ctx, 1, d, 32, 0, None) == BH_ERR_DEGREE_TOO_LARGE
    assert lib.bh_point_divide_by_z_on_coset_dev(worker.ctx, 1, d, 32, None) == BH_ERR_DEGREE_TOO_LARGE
    assert lib.bh_point_divide_by_z_on_coset_dev(worker.ctx, 5, d, 2, None) == BH_ERR_INVALID_ARG
    assert lib.bh_point_distribute_powers_dev(worker.ctx, 7, d, 4, _p(g), None) == BH_ERR_INVALID_ARG
    assert lib.bh_point_mul_assign_dev(worker.ctx, 0, d, d, 4, None) == BH_ERR_INVALID_ARG
    assert lib.bh_point_sub_assign_dev(worker.ctx, 9, d, d, 4, None) == BH_ERR_INVALID_ARG
    # n = 0 does nothing
    assert lib.bh_point_distribute_powers_dev(worker.ctx, 1, None, 0, _p(g), None) == 0
    assert lib.bh_point_mul_assign_dev(worker.ctx, 1, None, None, 0, None) == 0
    assert lib.bh_point_sub_assign_dev(worker.ctx, 2, None, None, 0, None) == 0
    worker.free(d)
    with pytest.raises(ValueError):
        bellman_amd.PointEvaluationDomain.from_coeffs(worker, 3, np.zeros((1, 12), dtype=np.uint64))

