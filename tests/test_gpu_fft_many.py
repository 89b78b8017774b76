"""k Fr vectors per call (bh_fft_fr_many_*, bh_h_poly_fr_many_dev_on, EvaluationDomains) on the GPU - src/domain.rs:81-125,
groth16/src/prover.rs:221-240.  Every vector j of a case is a different seeded random vector, so a swap of two vectors is
caught; the batched launches are forced (BH_FFT_MANY_FORCE) unless a test says otherwise.  Checked against the restated
best_fft per vector (oracle/c) at the sizes where the packing changes (V = 2^(11 - log_n) vectors per tile: k around V and
2V), at 2^11 (one vector per tile), at 2^12 / 2^13 on both table kinds, and byte for byte against k single-vector calls
where the oracle would take minutes (2^16 ... 2^25)."""

import ctypes

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

FORCE, SINGLE = 1, 2
OK, DEGREE_TOO_LARGE, INVALID_ARG = 0, 3, -2
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
TAIL = 64
MODES = ("fft", "ifft", "coset_fft", "icoset_fft")


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def worker_two_level():
    """a fresh context whose FFT table cache has no budget: every size runs on the two-level tables"""
    import bellman_amd

    w = bellman_amd.Worker(0)
    w.set_limits(fft_table_budget_bytes=0)
    yield w
    w.close()


def _lib():
    from bellman_amd import _lib as L

    return L.load()


def _at(dev, byte_offset):
    return ctypes.c_void_p(dev.value + byte_offset)


_VEC, _REF = {}, {}


def _vector(log_n, j):
    if (log_n, j) not in _VEC:
        _VEC[log_n, j] = cref.random_fr(1 << log_n, seed=100003 * log_n + j)
    return _VEC[log_n, j]


def _reference(log_n, mode, j):
    """computed once per (size, mode, vector) and shared by every test"""
    if (log_n, mode, j) not in _REF:
        _REF[log_n, mode, j] = cref.fft(_vector(log_n, j), mode)
    return _REF[log_n, mode, j]


def _layout(vectors, stride, tail=TAIL):
    k, n = len(vectors), vectors[0].shape[0]
    host = np.full((k * stride + tail, 4), SENTINEL, dtype=np.uint64)
    for j, v in enumerate(vectors):
        host[j * stride: j * stride + n] = v
    return host


def _run(worker, vectors, log_n, mode, flags=FORCE, gap=0, scratch_vectors=None):
    """the k vectors a stride apart in a sentinel-filled buffer through one call; returns the k results after checking that
    the gaps and the TAIL elements behind the last vector still hold the sentinel.  scratch_vectors: through the _on call
    with a scratch of that many vectors, else through bh_fft_fr_many_dev."""
    lib, k, n = _lib(), len(vectors), 1 << log_n
    stride = n + gap
    host = _layout(vectors, stride)
    dev = worker.alloc(host.nbytes)
    scratch = None
    try:
        worker.upload(dev, host)
        if scratch_vectors is None:
            rc = lib.bh_fft_fr_many_dev(worker.ctx, dev, stride * 32, k, log_n, mode, flags, None)
        else:
            scratch = worker.alloc(scratch_vectors * n * 32)
            rc = lib.bh_fft_fr_many_dev_on(worker.ctx, dev, stride * 32, k, log_n, mode, flags, scratch, scratch_vectors * n * 32, None)
        assert rc == OK, rc
        worker.synchronize()
        out = np.empty_like(host)
        worker.download(out, dev)
    finally:
        worker.free(dev)
        if scratch is not None:
            worker.free(scratch)
    for j in range(k):
        assert (out[j * stride + n: (j + 1) * stride] == SENTINEL).all(), "the gap behind vector %d was written" % j
    assert (out[k * stride:] == SENTINEL).all(), "the elements behind the last vector were written"
    return [out[j * stride: j * stride + n] for j in range(k)]


def _check_against_oracle(worker, log_n, k, mode, **kw):
    got = _run(worker, [_vector(log_n, j) for j in range(k)], log_n, mode, **kw)
    for j in range(k):
        assert np.array_equal(got[j], _reference(log_n, mode, j)), (log_n, k, MODES[mode], j, kw)


def _packed_ks(log_n):
    V = 1 << (11 - log_n)
    return sorted({min(k, 67) for k in (1, V - 1, V, V + 1, 2 * V + 3) if k >= 1})


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 8, 10])
def test_packed_sizes_match_the_oracle(worker, log_n, mode):
    """(2^2: a tile of 512 columns over 256 threads - a thread's elements alternate between two columns, so a partly filled
    tile has live and dead elements interleaved within a thread)"""
    for k in _packed_ks(log_n):
        _check_against_oracle(worker, log_n, k, mode)


@pytest.mark.parametrize("mode", range(4))
def test_one_vector_per_tile_matches_the_oracle(worker, mode):
    for k in (1, 4, 5):
        _check_against_oracle(worker, 11, k, mode)


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("log_n", [12, 13])
@pytest.mark.parametrize("tables", ["one_level", "two_level"])
def test_two_pass_sizes_match_the_oracle_on_both_table_kinds(worker, worker_two_level, tables, log_n, mode):
    w = worker if tables == "one_level" else worker_two_level
    for k in (1, 2, 5):
        _check_against_oracle(w, log_n, k, mode)


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("log_n,k", [(3, 67), (10, 3), (11, 5), (12, 5), (13, 2)])
def test_gaps_between_vectors_are_not_touched(worker, log_n, k, mode):
    """stride = n + 3 elements: the gaps and 64 elements behind the last vector keep their sentinel (checked in _run)"""
    _check_against_oracle(worker, log_n, k, mode, gap=3)


@pytest.mark.parametrize("scratch_vectors", [1, 2, 5])
def test_sub_batches_through_a_small_scratch(worker, scratch_vectors):
    """2^12 x 5 through the _on call: 5, 3 and 1 sub-batches"""
    for mode in range(4):
        _check_against_oracle(worker, 12, 5, mode, scratch_vectors=scratch_vectors)


def _powers(worker, dev, n, j):
    """vector j of a large case, made on the device: (j + 3) * g_j^i with a different g per vector"""
    from bellman_amd.groth16 import fr_to_mont_array

    gs = fr_to_mont_array([0x9E3779B97F4A7C15 + 2 * j, j + 3])
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert _lib().bh_fr_powers_dev(worker.ctx, dev, n, p(gs[0:1]), p(gs[1:2]), None) == OK


@pytest.mark.parametrize("log_n,k", [(16, 5), (21, 3), (23, 2), (25, 2)])
def test_large_sizes_equal_k_single_calls(worker, log_n, k):
    """byte for byte against bh_fft_fr_dev per vector: 2^16, 2^21 (tiles one and two elements wide), 2^23 (three passes),
    2^25 (above the one-level range)"""
    lib, n = _lib(), 1 << log_n
    vec = n * 32
    many, single = worker.alloc(k * vec), worker.alloc(k * vec)
    try:
        for mode in (0, 3):
            for j in range(k):
                _powers(worker, _at(many, j * vec), n, j)
                _powers(worker, _at(single, j * vec), n, j)
            assert lib.bh_fft_fr_many_dev(worker.ctx, many, vec, k, log_n, mode, FORCE, None) == OK
            for j in range(k):
                assert lib.bh_fft_fr_dev(worker.ctx, _at(single, j * vec), log_n, mode, None) == OK
            worker.synchronize()
            a, b = np.empty((n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)
            for j in range(k):
                worker.download(a, _at(many, j * vec))
                worker.download(b, _at(single, j * vec))
                assert np.array_equal(a, b), (log_n, MODES[mode], j)
            assert not np.array_equal(a[:64], np.zeros((64, 4), dtype=np.uint64))
    finally:
        worker.free(many)
        worker.free(single)


@pytest.mark.parametrize("log_n", [3, 12])
def test_flags_give_the_same_bytes(worker, log_n):
    k = 5
    vectors = [_vector(log_n, j) for j in range(k)]
    for mode in range(4):
        forced = _run(worker, vectors, log_n, mode, flags=FORCE, gap=3)
        for flags in (0, SINGLE):
            got = _run(worker, vectors, log_n, mode, flags=flags, gap=3)
            assert all(np.array_equal(g, f) for g, f in zip(got, forced)), (log_n, MODES[mode], flags)
        assert np.array_equal(forced[4], _reference(log_n, mode, 4))


def test_host_call_transforms_contiguous_vectors(worker):
    log_n, k = 9, 5
    host = np.ascontiguousarray(np.stack([_vector(log_n, j) for j in range(k)]))
    assert _lib().bh_fft_fr_many(worker.ctx, host.ctypes.data_as(ctypes.c_void_p), k, log_n, 2) == OK
    for j in range(k):
        assert np.array_equal(host[j], _reference(log_n, 2, j))


def test_error_codes(worker):
    lib, ctx = _lib(), worker.ctx
    n12 = 1 << 12
    host = np.full((2 * n12 + TAIL, 4), SENTINEL, dtype=np.uint64)
    dev, scratch = worker.alloc(host.nbytes), worker.alloc(n12 * 32)
    try:
        worker.upload(dev, host)
        on = lambda *a: lib.bh_fft_fr_many_dev_on(*a)  # noqa: E731
        # log_n >= 32 first, whatever else is wrong
        assert on(ctx, dev, 32, 1, 32, 0, 0, None, 0, None) == DEGREE_TOO_LARGE
        assert on(None, None, 0, 1, 32, 9, 8, None, 0, None) == DEGREE_TOO_LARGE
        assert lib.bh_fft_fr_many_dev(None, None, 0, 1, 40, 9, 8, None) == DEGREE_TOO_LARGE
        assert lib.bh_fft_fr_many(None, None, 1, 32, 0) == DEGREE_TOO_LARGE
        assert lib.bh_h_poly_fr_many_dev_on(None, None, None, None, 0, 1, 32, 0, None, 0, None) == DEGREE_TOO_LARGE
        ok = (ctx, dev, n12 * 32, 2, 12, 0, FORCE, scratch, n12 * 32, None)
        bad = {
            "null ctx": (0, None), "null data": (1, None), "mode -1": (5, -1), "mode 4": (5, 4),
            "stride below a vector": (2, n12 * 32 - 32), "stride not a multiple of 32": (2, n12 * 32 + 8),
            "unknown flag": (6, 4), "unknown flag beside a known one": (6, FORCE | 8),
            "null scratch above 2^11": (7, None), "scratch below one vector": (8, n12 * 32 - 32),
        }
        for what, (i, v) in bad.items():
            args = list(ok)
            args[i] = v
            assert on(*args) == INVALID_ARG, what
            if i <= 6:
                assert lib.bh_fft_fr_many_dev(*(args[:7] + [None])) == INVALID_ARG, what
                h = (args[0], args[1], dev, dev, args[2], 2, 12, args[6], scratch, n12 * 32, None)
                if i != 5:
                    assert lib.bh_h_poly_fr_many_dev_on(*h) == INVALID_ARG, what
        assert lib.bh_h_poly_fr_many_dev_on(ctx, dev, None, dev, n12 * 32, 2, 12, 0, scratch, n12 * 32, None) == INVALID_ARG
        assert lib.bh_h_poly_fr_many_dev_on(ctx, dev, dev, None, n12 * 32, 2, 12, 0, scratch, n12 * 32, None) == INVALID_ARG
        assert lib.bh_h_poly_fr_many_dev_on(ctx, dev, dev, dev, n12 * 32, 2, 12, 0, None, 0, None) == INVALID_ARG
        assert lib.bh_fft_fr_many(None, None, 1, 3, 0) == INVALID_ARG
        assert lib.bh_fft_fr_many(ctx, host.ctypes.data_as(ctypes.c_void_p), 1, 3, 4) == INVALID_ARG
        # a single-pass size needs no scratch; k = 0 launches nothing and is no error even above 2^11
        assert on(ctx, dev, (1 << 11) * 32, 0, 11, 0, FORCE, None, 0, None) == OK
        for flags in (0, FORCE, SINGLE):
            assert on(ctx, dev, n12 * 32, 0, 12, 1, flags, scratch, n12 * 32, None) == OK
            assert lib.bh_fft_fr_many_dev(ctx, dev, n12 * 32, 0, 12, 1, flags, None) == OK
            assert lib.bh_h_poly_fr_many_dev_on(ctx, dev, dev, dev, n12 * 32, 0, 12, flags, scratch, n12 * 32, None) == OK
        assert lib.bh_fft_fr_many(ctx, host.ctypes.data_as(ctypes.c_void_p), 0, 12, 1) == OK
        worker.synchronize()
        out = np.empty_like(host)
        worker.download(out, dev)
        assert (out == SENTINEL).all(), "a refused call or k = 0 wrote to the buffer"
    finally:
        worker.free(dev)
        worker.free(scratch)


_H = {}


def _h_case(log_m, j):
    """a, b, c of witness j and the oracle's m - 1 quotient coefficients"""
    if (log_m, j) not in _H:
        m = 1 << log_m
        a, b, c = (cref.random_fr(m, seed=7000 * log_m + 10 * j + t) for t in range(3))
        _H[log_m, j] = (a, b, c, cref.h_coeffs(a, b, c))
    return _H[log_m, j]


@pytest.mark.parametrize("log_m", [3, 11, 12, 13])
def test_h_block_matches_the_oracle_and_the_single_call(worker, log_m):
    lib, m = _lib(), 1 << log_m
    vec = m * 32
    for k in (1, 3, 5):
        cases = [_h_case(log_m, j) for j in range(k)]
        stride = m + 3
        hosts = [_layout([cs[t] for cs in cases], stride) for t in range(3)]
        devs = [worker.alloc(h.nbytes) for h in hosts]
        scratch = worker.alloc(k * vec)
        one = [worker.alloc(vec) for _ in range(4)]
        try:
            for d, h in zip(devs, hosts):
                worker.upload(d, h)
            assert lib.bh_h_poly_fr_many_dev_on(worker.ctx, devs[0], devs[1], devs[2], stride * 32, k, log_m, FORCE, scratch, k * vec, None) == OK
            worker.synchronize()
            out = np.empty_like(hosts[0])
            worker.download(out, devs[0])
            for j in range(k):
                assert (out[j * stride + m: (j + 1) * stride] == SENTINEL).all()
            assert (out[k * stride:] == SENTINEL).all()
            for t in (1, 2):   # b and c are clobbered, their gaps are not
                bc = np.empty_like(hosts[t])
                worker.download(bc, devs[t])
                for j in range(k):
                    assert (bc[j * stride + m: (j + 1) * stride] == SENTINEL).all()
                assert (bc[k * stride:] == SENTINEL).all()
            for j in range(k):
                got = out[j * stride: j * stride + m]
                assert np.array_equal(got[: m - 1], cases[j][3]), (log_m, k, j)
                for t in range(3):
                    worker.upload(one[t], np.ascontiguousarray(cases[j][t]))
                assert lib.bh_h_poly_fr_dev_on(worker.ctx, one[0], one[1], one[2], one[3], log_m, None) == OK
                worker.synchronize()
                want = np.empty((m, 4), dtype=np.uint64)
                worker.download(want, one[0])
                assert np.array_equal(got, want), "all m words are the single call's"
        finally:
            for d in devs + [scratch] + one:
                worker.free(d)


def test_h_poly_many_mirror(worker):
    import bellman_amd

    log_m, k = 11, 3
    cases = [_h_case(log_m, j) for j in range(k)]
    got = bellman_amd.h_poly_many(worker, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], flags=FORCE)
    assert len(got) == k
    for j in range(k):
        assert got[j].shape == ((1 << log_m) - 1, 4) and np.array_equal(got[j], cases[j][3])
    assert bellman_amd.h_poly_many(worker, [], [], []) == []


def test_evaluation_domains(worker):
    import bellman_amd
    from bellman_amd import EvaluationDomain, EvaluationDomains

    log_n, n = 8, 256
    full = [_vector(log_n, j) for j in range(3)]
    coeffs = [full[0], full[1][:200], full[2][:129]]          # unequal lengths that pad to one m
    d = EvaluationDomains.from_coeffs(worker, coeffs)
    assert len(d) == 3 and d.m == n and d.exp == log_n
    padded = [np.vstack([c, np.zeros((n - c.shape[0], 4), dtype=np.uint64)]) for c in coeffs]
    assert all(np.array_equal(x, y) for x, y in zip(d.as_ref(), padded))
    with pytest.raises(ValueError):
        EvaluationDomains.from_coeffs(worker, [full[0], full[1][:128]])
    with pytest.raises(bellman_amd.PolynomialDegreeTooLarge):
        # (2^32 + 1 coefficients as a broadcast view: no memory behind it)
        EvaluationDomains.from_coeffs(worker, [np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), ((1 << 32) + 1, 4))])
    # a round trip, and each transform against the singular class
    d.ifft(flags=FORCE)
    d.fft(flags=FORCE)
    assert all(np.array_equal(x, y) for x, y in zip(d.as_ref(), padded))
    for name in MODES:
        getattr(d, name)(flags=FORCE)
        singles = []
        for j in range(3):
            s = EvaluationDomain.from_coeffs(worker, padded[j])
            getattr(s, name)()
            singles.append(s.into_coeffs())
        assert all(np.array_equal(x, y) for x, y in zip(d.as_ref(), singles)), name
        padded = singles
    # the pointwise operations against the singular class
    other = EvaluationDomains.from_coeffs(worker, [full[2], full[0], full[1]])
    want = []
    for j in range(3):
        s = EvaluationDomain.from_coeffs(worker, padded[j])
        o = EvaluationDomain.from_coeffs(worker, [full[2], full[0], full[1]][j])
        s.mul_assign(worker, o)
        s.sub_assign(worker, o)
        s.divide_by_z_on_coset()
        want.append(s.into_coeffs())
        o.into_coeffs()
    d.mul_assign(worker, other)
    d.sub_assign(worker, other)
    d.divide_by_z_on_coset()
    other.into_coeffs()
    got = d.into_coeffs()
    assert len(got) == 3 and all(np.array_equal(x, y) for x, y in zip(got, want))

