"""The batched transform's geometry (tests/models/ntt_many_model.py: packed tiles for single-pass sizes, (tile, vector)
grids with a scratch of S vectors above) against a plain DFT per vector over a toy field, with the tile shrunk so that
every plan is reachable at Python speed - and the launches the library itself plans (bh_test_fft_many_plan, host only)
replayed through the same coverage check and compared with a restatement of the sizes."""

import ctypes
import random

import numpy as np
import pytest

from oracle.pyref.engines import DummyEngine
from tests.models import ntt_many_model as mm
from tests.models.ntt_model import plan_passes

F = DummyEngine.Fr            # F_64513: 2-adicity 10, domains up to 2^9
LOG_TILE, MAX_R, THREADS = 4, 4, 2
GAP = 3


def _omega(log_n):
    w = F.ROOT_OF_UNITY
    for _ in range(log_n, F.S):
        w = w * w % F.r
    return w


_VECS, _REFS = {}, {}


def _vector(log_n, j):
    if (log_n, j) not in _VECS:
        rnd = random.Random(1000 * log_n + j)
        _VECS[log_n, j] = [rnd.randrange(F.r) for _ in range(1 << log_n)]
    return _VECS[log_n, j]


def _reference(log_n, mode, j):
    if (log_n, mode, j) not in _REFS:
        _REFS[log_n, mode, j] = mm.plain_dft(_vector(log_n, j), F.r, _omega(log_n), mode, F.MULTIPLICATIVE_GENERATOR)
    return _REFS[log_n, mode, j]


def _ks(log_n):
    V = 1 << (LOG_TILE - log_n) if log_n <= MAX_R else 1
    return sorted({k for k in (1, V - 1, V, V + 1, 2 * V + 3) if k >= 1})


@pytest.mark.parametrize("gap", [0, GAP])
@pytest.mark.parametrize("log_n", range(0, 2 * MAX_R + 2))
def test_model_matches_plain_dft_per_vector(log_n, gap):
    n, stride = 1 << log_n, (1 << log_n) + gap
    L = len(plan_passes(log_n, MAX_R))
    for k in _ks(log_n):
        for scratch_vectors in ([0] if L == 1 else sorted({1, 2, k})):
            plan = mm.many_plan(log_n, k, stride, scratch_vectors, False, LOG_TILE, MAX_R, threads=(THREADS, THREADS))
            mm.check_plan_coverage(plan, log_n, k, stride, scratch_vectors, LOG_TILE, MAX_R, threads=(THREADS, THREADS))
            for mode in range(4):
                mem = [None] * (k * stride + 64)      # None: the gaps and what lies behind the last vector
                for j in range(k):
                    mem[j * stride: j * stride + n] = _vector(log_n, j)
                scratch = [None] * (max(scratch_vectors, 1) * n)
                trace = {}
                mm.run_many(mem, scratch, plan, F.r, _omega(log_n), log_n, mode, LOG_TILE, MAX_R, THREADS,
                            gen=F.MULTIPLICATIVE_GENERATOR, trace=trace)
                for j in range(k):
                    assert mem[j * stride: j * stride + n] == _reference(log_n, mode, j), (log_n, k, mode, j, scratch_vectors)
                    assert all(v is None for v in mem[j * stride + n: (j + 1) * stride]), "a gap was written"
                assert all(v is None for v in mem[k * stride:])
                # every (vector, element) loaded exactly once by a first pass, stored exactly once by a last pass, and
                # nothing outside a vector touched: the trace of what the model did, element by element
                want = sorted(j * stride + i for j in range(k) for i in range(n))
                assert sorted(a for buf, a, op in trace[0] if op == "ld") == want and all(buf == "mem" for buf, a, op in trace[0] if op == "ld")
                assert sorted(a for buf, a, op in trace[L - 1] if op == "st") == want
                assert all(buf == "mem" for buf, a, op in trace[L - 1] if op == "st")
                for p in range(L):
                    for buf, a, op in trace[p]:
                        if buf == "scratch":
                            assert 0 <= a < max(scratch_vectors, 1) * n
                        else:
                            assert a % stride < n and a // stride < k


def test_block_order_keeps_a_tile_on_one_xcd():
    """(tile, vector) blocks: with the XCD-aware tile order (blocks b, b + 8, ... share an XCD) the n_vec workgroups of a tile
    have one b & 7 and consecutive b >> 3; without it they are consecutive blocks"""
    for grid_tiles, nv, swz in ((64, 5, 1), (1024, 3, 1), (4, 5, 0), (32, 2, 0)):
        grid = grid_tiles * nv
        where = {}
        for b in range(grid):
            t, v = mm.many_block(b, grid, nv, swz)
            where.setdefault(t, []).append((b, v))
        assert sorted(where) == list(range(grid_tiles))
        for t, bs in where.items():
            assert [v for _, v in bs] == list(range(nv))
            if swz:
                assert len({b & 7 for b, _ in bs}) == 1 and [b >> 3 for b, _ in bs] == list(range(bs[0][0] >> 3, (bs[0][0] >> 3) + nv))
            else:
                assert [b for b, _ in bs] == list(range(bs[0][0], bs[0][0] + nv))


def _library_plan(lib, log_n, k, stride, scratch_vectors, kind):
    cap = 256
    out = np.zeros((cap, 20), dtype=np.uint64)
    got = lib.bh_test_fft_many_plan(log_n, k, stride, scratch_vectors, kind, out.ctypes.data_as(ctypes.c_void_p), cap)
    assert 0 <= got <= cap, got
    return [dict(zip(mm.FIELDS, (int(x) for x in row))) for row in out[:got]]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("log_n", [0, 3, 10, 11, 12, 13, 21, 22, 23, 25])
def test_library_plan_replays(log_n, kind):
    """the launches bh_fft_fr_many_dev_on would issue (host only, no GPU), for both table kinds"""
    from bellman_amd import _lib
    lib = _lib.load()
    n = 1 << log_n
    one_level = kind == 1 and 12 <= log_n <= 24
    for k in (1, 2, 5, 33):
        for scratch_vectors in sorted({1, 2, k}):
            for stride in (n, n + GAP):
                plan = _library_plan(lib, log_n, k, stride, scratch_vectors, kind)
                assert plan == mm.many_plan(log_n, k, stride, scratch_vectors, one_level), (log_n, k, scratch_vectors, stride)
                mm.check_plan_coverage(plan, log_n, k, stride, scratch_vectors)
                L = len(plan_passes(log_n))
                subs = 1 if L == 1 else -(-k // scratch_vectors)
                assert len(plan) == subs * L
                assert all(l["one_level"] == int(one_level) for l in plan)


def test_library_plan_refuses():
    from bellman_amd import _lib
    lib = _lib.load()
    out = np.zeros((4, 20), dtype=np.uint64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.bh_test_fft_many_plan(32, 1, 1 << 32, 1, 0, p, 4) < 0          # no such domain
    assert lib.bh_test_fft_many_plan(12, 2, (1 << 12) - 1, 1, 0, p, 4) < 0     # vectors would overlap
    assert lib.bh_test_fft_many_plan(12, 2, 1 << 12, 0, 0, p, 4) < 0           # a multi-pass size needs a scratch vector
    assert lib.bh_test_fft_many_plan(11, 2, 1 << 11, 0, 0, p, 4) == 1          # a single-pass size does not
    assert lib.bh_test_fft_many_plan(3, 0, 8, 0, 0, p, 4) == 0                 # k = 0: nothing to launch
