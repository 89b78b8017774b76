"""The window table of a base vector as bh_bases_precompute builds it: ONE pass of window_table_kernel (csrc/point_kernels.cuh)
that writes every row at the stride the table keeps - through bh_test_window_table_dev, which builds into a buffer filled
with a sentinel byte and followed by a guard and returns both raw (run with `pytest -m gpu` on a MI355X).

  * G1 at the dense stride (96) and at 128 bytes, G2 at 192; n = 1, 127, 129 (129: two workgroups, the second with one live
    lane); c = 13 and 20 (20 and 13 rows); identity records at index 0 and n - 1;
  * row 0 is the input; at stride 128 the 96 record bytes equal the dense build and the 32 bytes between two records, like
    the guard, are never written;
  * row j record i == the oracle's [2^(c j)] P_i as field elements mod p, identity to identity;
  * the books of the context's table budget (bh_ctx_info table_bytes) return to where they started after register ->
    explicit precompute -> release, and after register -> trim.
Integer work: no tolerances."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_groth16 import worker  # noqa: E402,F401

SHAPES = [(1, 96), (1, 128), (2, 192)]     # (group, stride)
REC = {1: 96, 2: 192}


@pytest.fixture(scope="module")
def hook():
    from bellman_amd import _lib

    lib = _lib.load()
    shape = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(0, 0, shape) == 0
    return lib, int(shape[7]), int(shape[11])   # guard bytes, sentinel byte


_POINTS, _TABLES = {}, {}


def points(group, n):
    """n records with the identity at index 0 and at index n - 1 (a lone record stays a point: see the test below)"""
    if (group, n) not in _POINTS:
        from oracle import cref

        pts = cref.gen_bases(group, n, a=7, b=11)
        if n > 1:
            pts[0] = 0
            pts[n - 1] = 0
        _POINTS[group, n] = pts
    return _POINTS[group, n]


def build(hook, worker, group, pts, stride, c):
    """(records [W n, stride] as bytes, guard bytes) of one build"""
    lib, guard, _ = hook
    n, W = pts.shape[0], (256 + c - 1) // c
    out = np.zeros(W * n * stride + guard, dtype=np.uint8)
    rc = lib.bh_test_window_table_dev(worker.ctx, group, pts.ctypes.data_as(ctypes.c_void_p), n, stride, c,
                                      out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (group, n, stride, c, rc)
    return out[: W * n * stride].reshape(W * n, stride), out[W * n * stride:]


def table(hook, worker, group, n, stride, c):
    key = (group, n, stride, c)
    if key not in _TABLES:
        _TABLES[key] = build(hook, worker, group, points(group, n), stride, c)
    return _TABLES[key]


@pytest.mark.parametrize("c", [13, 20])
@pytest.mark.parametrize("n", [1, 127, 129])
@pytest.mark.parametrize("group,stride", SHAPES)
def test_rows_sit_at_the_stride_and_nothing_else_is_written(hook, worker, group, stride, n, c):
    sentinel = hook[2]
    rec = REC[group]
    recs, guard = table(hook, worker, group, n, stride, c)
    pts = points(group, n)
    assert np.array_equal(recs[:n, :rec], pts.view(np.uint8).reshape(n, rec))            # row 0 is the input
    assert np.all(guard == sentinel)
    if stride != rec:
        dense, _ = table(hook, worker, group, n, rec, c)
        assert np.array_equal(recs[:, :rec], dense)                                        # the same table, byte for byte
        assert np.all(recs[:, rec:] == sentinel)                                           # pad bytes: never written
    if n > 1:   # an identity stays the identity in every row
        rows = recs[:, :rec].reshape(-1, n, rec)
        assert not rows[:, 0].any() and not rows[:, n - 1].any() and rows[:, 1].any(axis=1).all()


@pytest.mark.parametrize("group", [1, 2])
def test_a_lone_identity_record(hook, worker, group):
    pts = np.zeros((1, REC[group] // 8), dtype=np.uint64)
    recs, guard = build(hook, worker, group, pts, REC[group], 13)
    assert not recs.any() and np.all(guard == hook[2])


@pytest.mark.parametrize("group,stride,n,c", [(1, 128, 129, 20), (2, 192, 127, 13)])
def test_rows_are_the_multiples_of_the_oracle(hook, worker, group, stride, n, c):
    from oracle import cref

    rec, W = REC[group], (256 + c - 1) // c
    recs, _ = table(hook, worker, group, n, stride, c)
    got = np.ascontiguousarray(recs[:, :rec]).view(np.uint64).reshape(W, n, rec // 8)
    want = points(group, n).copy()
    for j in range(W):
        if j:   # [2^(c j)] P_i = [2^c] of the row before
            want = np.stack([cref.point_mul(group, p, 1 << c) for p in want])
        for i in range(n):
            g = [v % cref.P for v in cref.arr_to_ints(got[j, i].reshape(-1, 6))]           # field elements mod p
            w = cref.arr_to_ints(want[i].reshape(-1, 6))
            assert g == w, (j, i)
            assert (not any(w)) == (i in (0, n - 1)), (j, i)                                # identity to identity, and only there


def test_hook_refuses_other_strides(hook, worker):
    lib = hook[0]
    out = np.zeros(1 << 20, dtype=np.uint8)
    for group, stride in ((1, 192), (1, 112), (1, 64), (2, 128), (2, 96), (2, 256)):
        pts = points(group, 127)
        assert lib.bh_test_window_table_dev(worker.ctx, group, pts.ctypes.data_as(ctypes.c_void_p), 127, stride, 13,
                                            out.ctypes.data_as(ctypes.c_void_p)) == -2, (group, stride)


def test_table_bytes_return_to_where_they_started():
    """register (automatic table: counted) -> bh_bases_precompute(16) (explicit: no longer counted) -> release, and
    register -> bh_ctx_trim: the context's table_bytes is back at its starting value each time, on a 2^10-point G1 vector"""
    import bellman_amd
    from oracle import cref

    pts = cref.gen_bases(1, 1 << 10, a=3, b=2)
    w = bellman_amd.Worker(0)
    try:
        start = w.info()["table_bytes"]
        hb = bellman_amd.Bases(w, 1, pts)
        c, rows, nbytes = hb.table_info()
        assert rows > 0 and nbytes == rows * (1 << 10) * 96 and w.info()["table_bytes"] == start + nbytes
        hb.precompute(16)
        assert hb.table_info() == (16, 16, 16 * (1 << 10) * 96) and w.info()["table_bytes"] == start
        hb.release()
        assert w.info()["table_bytes"] == start
        hb = bellman_amd.Bases(w, 1, pts)
        assert w.info()["table_bytes"] == start + nbytes
        w.trim()
        assert hb.table_info() == (0, 0, 0) and w.info()["table_bytes"] == start
        hb.release()
        assert w.info()["table_bytes"] == start
    finally:
        w.close()
