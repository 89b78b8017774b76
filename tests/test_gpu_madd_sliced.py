"""The mixed addition of the G1 bucket accumulation over sliced operands, on raw projective operands (`pytest -m gpu`).

ec.cuh xyzz_madd_sliced cuts every value of the addition into 30-bit limbs once and multiplies the limbs (ff.cuh fe_mul_hh,
fe_sqr_h, fe_mul2_hh); xyzz_madd cuts inside every product.  The claim is the SAME WORDS: bh_test_g1_madd_sliced_dev runs
xyzz_madd and the sliced addition on each case, and the two raw records are compared word for word; the device run is
compared with the same function compiled for the host, and xyzz_madd's result with the affine model.

Cases: the whole madd table of tests/group_model (general, acc == q, acc == -q, identity accumulators clean and dirty,
identity bases; representations with l = 1 - ZZ = ZZZ = 1, the accumulator right after an opener -, l = p - 1, residues
with every limb near its maximum, coefficients written as v + p), and records that no curve point has, where the formula
is plain arithmetic: every coordinate of the accumulator and of the base at p - 1, at 2p - 1 (accumulator), at 1, at the
Montgomery one."""

import numpy as np
import pytest

from tests import group_model as gm

pytestmark = pytest.mark.gpu

FORM, OP = 0, gm.OP["madd"]
P = gm.P


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def corner_records():
    """(a, q) pairs off the curve: the products and subtractions see the extreme words"""
    vals_a = [P - 1, 2 * P - 1, 1, gm.ONE, P + 1]
    vals_q = [P - 1, 1, gm.ONE, P - 2]
    out = []
    for va in vals_a:
        for vq in vals_q:
            out.append(((va,) * 4, (vq, vq)))
    # mixed: X, Y at p - 1 with ZZ = ZZZ = 1 (Montgomery), and the other way round
    out.append(((P - 1, P - 1, gm.ONE, gm.ONE), (P - 1, P - 1)))    # U2 = X1, S2 = Y1: the doubling branch on p - 1
    out.append(((P - 1, 1, gm.ONE, gm.ONE), (P - 1, P - 1)))        # U2 = X1, S2 != Y1: the inverse branch
    out.append(((gm.ONE, gm.ONE, P - 1, P - 1), (P - 1, P - 1)))
    return out


@pytest.fixture(scope="module")
def operands():
    table = gm.operands_for((FORM, OP, 0))
    a, q = gm.operand_arrays(FORM, OP, table)
    extra = corner_records()
    a = np.concatenate([a, gm._pack([c[0] for c in extra])])
    q = np.concatenate([q, gm._pack([c[1] for c in extra])])
    return table, np.ascontiguousarray(a), np.ascontiguousarray(q)


def run_host(lib, a, q):
    n = a.shape[0]
    raw = np.zeros((2 * n, a.shape[1]), dtype=np.uint8)
    flags = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    assert lib.bh_test_g1_madd_sliced_host(gm._ptr(raw), gm._ptr(flags), gm._ptr(a), gm._ptr(q), n) == 0
    return raw, flags


def run_dev(lib, worker, a, q):
    n, rbytes = a.shape
    raw = np.zeros(2 * n * rbytes + gm.GUARD, dtype=np.uint8)
    raw[2 * n * rbytes:] = 0xA5
    flags = np.full(n + gm.GUARD // 4, 0xA5A5A5A5, dtype=np.uint32)
    bufs = []
    try:
        dev = []
        for arr in (a, q, raw, flags):
            d = worker.alloc(arr.nbytes)
            bufs.append(d)
            worker.upload(d, arr)
            dev.append(d)
        assert lib.bh_test_g1_madd_sliced_dev(worker.ctx, dev[2], dev[3], dev[0], dev[1], n) == 0
        worker.download(raw, dev[2])
        worker.download(flags, dev[3])
    finally:
        for d in bufs:
            worker.free(d)
    assert (raw[2 * n * rbytes:] == 0xA5).all() and (flags[n:] == 0xA5A5A5A5).all(), "bytes behind the results were written"
    return raw[:2 * n * rbytes].reshape(2 * n, rbytes), flags[:n]


def test_sliced_addition_gives_the_words_of_xyzz_madd(lib, worker, operands):
    table, a, q = operands
    n = a.shape[0]
    assert a.shape[1] == 192 and q.shape[1] == 96 and n > len(table) > 1000
    raw, flags = run_dev(lib, worker, a, q)
    ref, chk = raw[:n], raw[n:]
    bad = np.nonzero((ref != chk).any(axis=1))[0]
    assert bad.size == 0, "xyzz_madd_sliced differs from xyzz_madd at cases %s" % bad[:8]
    assert (((flags >> 0) & 1) == ((flags >> 1) & 1)).all()   # the return values agree
    res = gm._unpack(ref, n)
    # xyzz_madd itself against the affine model, on the curve cases
    seen = set()
    for i, c in enumerate(table):
        got = gm.decode(1, res[i])
        assert got == c.want, (i, c.cls)
        assert bool(flags[i] & 16) == (c.b == gm.affine_record(1, None)), i
        seen.add(c.cls)
    assert {"general", "same", "opposite", "a_identity", "dirty_identity", "b_identity"} <= seen
    # device == host, every word and flag
    hraw, hflags = run_host(lib, a, q)
    assert np.array_equal(hraw, raw) and np.array_equal(hflags, flags)


def test_table_has_the_named_operands(operands):
    """the cases the comparison is meant to include are in the table: ZZ = ZZZ = 1, l = p - 1, acc == q, acc == -q"""
    table, _, _ = operands
    one_reps = [c for c in table if c.cls in ("general", "same", "opposite") and c.a[2] % P == gm.ONE and c.a[3] % P == gm.ONE]
    assert one_reps
    assert any(c.cls == "same" for c in table) and any(c.cls == "opposite" for c in table)
    assert any(c.a[2] % P == gm.ONE and c.a[3] % P == P - gm.ONE for c in table)   # l = p - 1: ZZ = 1, ZZZ = -1
