"""The key-aware kernels of the calls over a bh_pvk_set, each on its own through its launch function and hook
(bh_test_pairing_*_keys_dev, include/bellman_hip_test.h), word for word against tests/models/pairing_stage_model.py.

One layout serves every test: three keys with 0, 2 and 16 inputs (window widths 8, 8 and 2) as four descriptors - the key
without inputs stands in the set twice - over 130 rows, so that the key boundaries fall at rows 1, 64 and 129: a block of
one row, a run that ends with its wave, a run of 65 rows cut into 64 + 1, and a last block of one row.  No tolerance
anywhere: integer work; every guard must come back untouched."""

import ctypes

import numpy as np
import pytest

from bellman_amd import _abi
from tests import field_model as fm
from tests import group_model as gm
from tests.models import pairing_stage_model as psm
from tests.models import verify_keys_model as vkm
from tests.test_gpu_pairing_stages import F12_BYTES, call, f12_at, lines_and_flags, out, table_rec, u32s

pytestmark = pytest.mark.gpu
P, Q = psm.P, psm.Q
N = 130
KEY_OF = [0] + [1] * 63 + [2] * 65 + [3]
KEY_BUFS = ("tables", "ic0", "key lines", "key flags", "f_ab", "alpha", "descriptors")


KeyLayout = _abi.STRUCTS["bh_test_key_layout"]


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load()


class Layout:
    """the four descriptors and what the hooks upload for them"""

    N_INPUTS = (0, 2, 16, 0)
    WIDTHS = (8, 8, 2, 8)

    def __init__(self):
        k0, k2, k16 = (psm.ScalarKey(n, "keys stages %d" % n) for n in (0, 2, 16))
        self.keys = [k0, k2, k16, k0]
        self.kflags = [[0, 0, 0], [psm.PF_IDENTITY, 0, 0], [0, 0, 0], [0, psm.PF_IDENTITY, 0]]   # (a flag switches the pair off)
        self.kq = [[gm.neg(2, k.gamma), gm.neg(2, k.delta), k.beta] for k in self.keys]
        rnd = psm.rng("keys stages f_ab")
        self.f_ab_raw = [psm.random_f12_lazy(rnd) for _ in range(3)]
        self.f_ab_raw.append(self.f_ab_raw[0])
        self.col_off = [0, 1, 4, 21]
        self.total_cols = 22
        self.perm, self.segs, self.blocks = vkm.group_rows(KEY_OF, self.N_INPUTS)
        assert self.perm == list(range(N))
        assert [b[1] for b in self.blocks] == [0, 1, 64, 128, 129] and [b[2] for b in self.blocks] == [1, 63, 64, 1, 1]
        self._tables = None

    def tables(self):
        if self._tables is None:
            self._tables = [psm.ic_table(k.ic[1:], w) for k, w in zip(self.keys, self.WIDTHS)]
        return self._tables

    def struct(self, *fields):
        """the layout with the named arrays (the others NULL) -> (structure, what must stay alive)"""
        data = {
            "n_inputs": u32s(self.N_INPUTS), "widths": u32s(self.WIDTHS),
            "tables": lambda: b"".join(table_rec(t) for t in self.tables()),
            "ic0": lambda: b"".join(psm.g1_rec(k.ic[0]) for k in self.keys),
            "lines": lambda: b"".join(psm.lines_rec(psm.g2_lines(q)) for qs in self.kq for q in qs),
            "qflags": lambda: u32s(f for fl in self.kflags for f in fl),
            "f_ab": lambda: b"".join(psm.fp_bytes(v) for raw in self.f_ab_raw for v in raw),
            "alpha": lambda: b"".join(psm.g1_rec(k.alpha) for k in self.keys),
        }
        s = KeyLayout()
        s.n_keys = 4
        keep = []
        for name in ("n_inputs", "widths") + fields:
            raw = data[name]() if callable(data[name]) else data[name]
            arr = np.frombuffer(raw, dtype=np.uint8).copy()
            keep.append(arr)
            setattr(s, name, arr.ctypes.data)
        return s, keep

    def blocks_raw(self):
        return u32s(v for b in self.blocks for v in b)


@pytest.fixture(scope="module")
def lay():
    return Layout()


def test_arguments_outside_a_buffer_are_refused(lib, worker, lay):
    g = np.zeros(16, dtype=np.uint32)
    b = bytes(1 << 16)
    s, keep = lay.struct("tables", "ic0", "lines", "qflags", "f_ab", "alpha")
    ref = ctypes.addressof(s)
    ctx = worker.ctx
    for blocks in ([(4, 0, 1, 0)], [(0, 0, 65, 0)], [(0, 0, 0, 0)], [(0, 129, 2, 0)], [(2, 0, 1, 1151)]):
        raw = u32s(v for blk in blocks for v in blk)
        assert lib.bh_test_pairing_ic_accumulate_keys_dev(ctx, ref, raw, 1, b, 1166, 0, N, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_ic_accumulate_keys_dev(ctx, ref, lay.blocks_raw(), 5, b, 1166, 2, N, b, g.ctypes.data) == -2
    s2, keep2 = lay.struct("tables")
    assert lib.bh_test_pairing_ic_accumulate_keys_dev(ctx, ctypes.addressof(s2), lay.blocks_raw(), 5, b, 1166, 0, N, b,
                                                      g.ctypes.data) == -2                                           # no ic0
    assert lib.bh_test_pairing_miller3_keys_dev(ctx, ctypes.addressof(s2), lay.blocks_raw(), 5, b, b, b, b, b, 1, N, b,
                                                g.ctypes.data) == -2                                                 # no lines
    assert lib.bh_test_pairing_fold3_const_keys_dev(ctx, ctypes.addressof(s2), lay.blocks_raw(), 5, b, N, 1, g.ctypes.data) == -2
    assert lib.bh_test_pairing_g1_mul_keys_dev(ctx, ctypes.addressof(s2), b, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_miller_keys_dev(ctx, ctypes.addressof(s2), b, b, g.ctypes.data) == -2
    segs = u32s([0, 1, 0, 0, 1, 63, 0, 0, 64, 67, 126, 0, 129, 1, 0, 0])                                             # rows past n
    assert lib.bh_test_pairing_colsum_keys_dev(ctx, ref, segs, b, b, 1166, 0, N, 0, b, b, g.ctypes.data) == -2
    s.n_keys = 65
    assert lib.bh_test_pairing_g1_mul_keys_dev(ctx, ref, b, b, g.ctypes.data) == -2
    del keep, keep2


# --------------------------------------------------------------------------------------------------- ic accumulation per key
@pytest.mark.parametrize("fmt", [psm.CANONICAL, psm.MONT])
def test_ic_accumulate_keys(lib, worker, lay, fmt):
    rnd = psm.rng("keys stages accumulate")
    edges = [0, 1, Q - 1]
    pool2 = [[edges[(t + i) % 3] if t < 3 else rnd.randrange(Q) for i in range(2)] for t in range(5)]
    pool16 = [[edges[(t + i) % 3] if t < 2 else rnd.randrange(Q) for i in range(16)] for t in range(3)]
    if fmt == psm.CANONICAL:   # values >= q are used as they are
        pool2.append([Q, (1 << 256) - 1])
        pool16.append([pool16[2][i] + Q if i % 2 else pool16[2][i] for i in range(16)])
    rows = [[]] + [pool2[j % len(pool2)] for j in range(63)] + [pool16[(j + j // 64) % len(pool16)] for j in range(65)] + [[]]
    s, keep = lay.struct("tables", "ic0")
    res = out(N * 96)
    inputs = psm.fr_bytes(psm.scalar_raw(v, fmt) for row in rows for v in row)
    assert len(inputs) == 1166 * 32
    call(lib.bh_test_pairing_ic_accumulate_keys_dev, ("inputs", "blocks", "out") + KEY_BUFS, worker.ctx, ctypes.addressof(s),
         lay.blocks_raw(), len(lay.blocks), inputs, 1166, fmt, N, res.ctypes.data)
    for j, row in enumerate(rows):
        key = lay.keys[KEY_OF[j]]
        assert psm.decode_g1(res[j * 96:(j + 1) * 96]) == psm.ic_accumulate(key.ic[0], key.ic[1:], row), (fmt, j)
    del keep


# ---------------------------------------------------------------------------------------------------- three Miller loops
def miller3_lanes():
    g1, g2 = psm.g1_points(), psm.g2_points()
    a_pool = [g1["random"][0], g1["generator"][0], None]
    b_pool = [g2["generator"][0], g2["random"][0], None]
    acc_pool = [g1["random"][1], None, g1["generator"][0]]
    c_pool = [g1["random"][2], None]
    return [(a_pool[j % 3], b_pool[(j // 3) % 3], acc_pool[(j + j // 7) % 3], c_pool[(j // 2 + j // 9) % 2]) for j in range(N)]


@pytest.mark.parametrize("separate", [1, 0])
def test_miller3_keys(lib, worker, lay, separate):
    lanes = miller3_lanes()
    blines, bflags = lines_and_flags([b for _, b, _, _ in lanes], 1)
    s, keep = lay.struct("lines", "qflags")
    f = out((3 if separate else 1) * N * F12_BYTES)
    call(lib.bh_test_pairing_miller3_keys_dev, ("a", "acc", "proofs", "blines", "bflags", "blocks", "f") + KEY_BUFS, worker.ctx,
         ctypes.addressof(s), lay.blocks_raw(), len(lay.blocks), b"".join(psm.g1_rec(a) for a, _, _, _ in lanes),
         b"".join(psm.g1_rec(g) for _, _, g, _ in lanes), b"".join(psm.proof_rec(None, None, c) for _, _, _, c in lanes), blines,
         u32s(bflags), separate, N, f.ctypes.data)
    differ = 0
    for j, (a, b, g, c) in enumerate(lanes):
        k = KEY_OF[j]
        fl, kq = lay.kflags[k], lay.kq[k]
        want = [psm.miller(a, b), psm.miller(g, None if fl[0] & 1 else kq[0]), psm.miller(c, None if fl[1] & 1 else kq[1])]
        if separate:
            for y in range(3):
                assert f12_at(f, y * N + j) == want[y], (j, y)
        else:
            assert f12_at(f, j) == psm.f12_product(want), j
        differ += want[1] != fm.F12_ONE and want[2] != fm.F12_ONE
    assert differ > 10          # rows whose key pairs are both switched on
    del keep


def test_fold3_and_the_constant_of_the_rows_key(lib, worker, lay):
    rnd = psm.rng("keys stages fold3")
    s, keep = lay.struct("f_ab")
    for separate in (1, 0):
        k = 3 if separate else 1
        distinct = [psm.random_f12_lazy(rnd) for _ in range(7)]
        raws = [distinct[(i * 3 + i // 7) % 7] for i in range(k * N)]
        buf = np.frombuffer(b"".join(psm.fp_bytes(v) for raw in raws for v in raw), dtype=np.uint8).copy()
        call(lib.bh_test_pairing_fold3_const_keys_dev, ("f", "blocks") + KEY_BUFS, worker.ctx, ctypes.addressof(s), lay.blocks_raw(),
             len(lay.blocks), buf.ctypes.data, N, separate)
        for j in range(N):
            want = psm.f12_product([psm.f12_of_raw(raws[y * N + j]) for y in range(k)] + [psm.f12_of_raw(lay.f_ab_raw[KEY_OF[j]])])
            assert f12_at(buf, j) == want, (separate, j)
    assert psm.f12_of_raw(lay.f_ab_raw[1]) != psm.f12_of_raw(lay.f_ab_raw[2])
    del keep


# ------------------------------------------------------------------------------------------------- segmented column sums
@pytest.mark.parametrize("fmt,nb_override,last_key_empty", [(psm.CANONICAL, 0, False), (psm.MONT, 0, False), (psm.CANONICAL, 3, False),
                                                            (psm.MONT, 2, True)])
def test_colsum_keys(lib, worker, lay, fmt, nb_override, last_key_empty):
    rnd = psm.rng("keys stages colsum %d %d" % (fmt, nb_override))
    edges = [v for v in psm.FR_EDGES if fmt == psm.CANONICAL or v < Q]
    pool = [psm.scalar_raw(v, fmt) for v in edges] + [rnd.randrange(Q if fmt == psm.MONT else 1 << 256) for _ in range(40)]
    zpool = [r for r in pool if psm.scalar_int(r, fmt) % Q]
    n = N - 1 if last_key_empty else N
    z = [zpool[(j * 5) % len(zpool)] for j in range(n)]
    rows = [[pool[(j * 7 + i * 13) % len(pool)] for i in range(lay.N_INPUTS[KEY_OF[j]])] for j in range(n)]
    segs = [(first, count if first + count <= n else 0, scalar) for first, count, scalar in lay.segs]
    acc0 = [rnd.randrange(1, Q) for _ in range(lay.total_cols)]      # what earlier chunks left
    acc = np.frombuffer(psm.fr_bytes(v * psm.RQ % Q for v in acc0), dtype=np.uint8).copy()
    part = out(lay.total_cols * psm.COLSUM_BLOCKS * 32)
    s, keep = lay.struct()
    call(lib.bh_test_pairing_colsum_keys_dev, ("z", "inputs", "segs", "part", "acc") + KEY_BUFS, worker.ctx, ctypes.addressof(s),
         u32s(v for seg in segs for v in seg + (0,)), psm.fr_bytes(z), psm.fr_bytes(v for row in rows for v in row), 1166, fmt, n,
         nb_override, acc.ctypes.data, part.ctypes.data)
    nb = nb_override or 1                                             # the shipped rule: 65 rows at the most -> one block row
    got_acc, got_part = psm.words(acc, 32), psm.words(part, 32)
    assert all(v < Q for v in got_acc)
    for k, (first, count, _) in enumerate(segs):
        ncol = lay.N_INPUTS[k] + 1
        lo = lay.col_off[k]
        want_part, want_acc = psm.colsum(z[first:first + count], rows[first:first + count], ncol, acc0[lo:lo + ncol], fmt, nb)
        assert [v * fm.RQ_INV % Q for v in got_acc[lo:lo + ncol]] == want_acc, (k, "acc")
        for col in range(ncol):
            vals = got_part[(lo + col) * nb:(lo + col + 1) * nb]
            assert all(v < Q for v in vals) and [v * fm.RQ_INV % Q for v in vals] == want_part[col], (k, col)
        if not count:
            assert want_acc == acc0[lo:lo + ncol]
    assert psm.is_sentinel(part[lay.total_cols * nb * 32:])
    del keep


# ------------------------------------------------------------------------------------------------------ the batch's tail
def test_g1_mul_keys(lib, worker, lay):
    rnd = psm.rng("keys stages g1 mul")
    acc = [rnd.randrange(Q) for _ in range(lay.total_cols)]
    acc[lay.col_off[1]] = 0                                           # a key without a proof in the batch: the identity
    acc[lay.col_off[3]] = Q - 1
    s, keep = lay.struct("alpha")
    res = out(4 * 96)
    call(lib.bh_test_pairing_g1_mul_keys_dev, ("acc", "out") + KEY_BUFS, worker.ctx, ctypes.addressof(s),
         psm.fr_bytes(v * psm.RQ % Q for v in acc), res.ctypes.data)
    for k in range(4):
        want = psm.g1_mul(lay.keys[k].alpha, acc[lay.col_off[k]])
        assert psm.decode_g1(res[k * 96:(k + 1) * 96]) == want, k
    assert bytes(res[96:192]) == bytes(96)
    del keep


def test_miller_keys(lib, worker, lay):
    g1 = psm.g1_points()
    pts = [g1["random"][0], g1["generator"][0], None, g1["random"][1]]
    p = [pts[(which + k) % 4] for which in range(3) for k in range(4)]     # [which][key]
    s, keep = lay.struct("lines", "qflags")
    f = out(12 * F12_BYTES)
    call(lib.bh_test_pairing_miller_keys_dev, ("p", "f") + KEY_BUFS, worker.ctx, ctypes.addressof(s), b"".join(psm.g1_rec(x) for x in p),
         f.ctypes.data)
    ones = 0
    for which in range(3):
        for k in range(4):
            q = None if lay.kflags[k][which] & 1 else lay.kq[k][which]
            want = psm.miller(p[which * 4 + k], q)
            assert f12_at(f, which * 4 + k) == want, (which, k)
            ones += want == fm.F12_ONE
    assert ones == 5            # three identity points, two switched-off pairs, none of them twice
    del keep
