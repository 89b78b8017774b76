"""The G1 bucket accumulation with its Fp products inline, word for word against xyzz_madd (`pytest -m gpu`).

msm_accumulate_kernel<FpOps, false> runs ec.cuh xyzz_madd_sliced<FpOps, true>: every value cut into 30-bit limbs once and
the six products and two squarings of the add path inline (ff.cuh fp_mul_hh_inl, fp_sqr_h_inl).  The claim is that every
word it stores is the word xyzz_madd - unsliced, products out of line - stores.  Two entry points reach the shipped code:

  bh_test_bucket_stage_dev   launches the accumulation as msm_enqueue does.  Accumulate form 0 is the kernel above; form 1,
                             msm_accumulate_kernel<FpOps, true>, walks the same chunks with xyzz_madd.  Both run on the
                             same stream and the raw buckets, head slots, tail slots and counters are compared byte for
                             byte (the merge launches that follow see equal inputs, so the merged buckets are equal too).
  bh_test_g1_madd_sliced_dev one addition per case on raw operands: xyzz_madd next to the sliced inline addition.

Streams, each at c = 10 and 13 and K = 8 and 52 (a few thousand entries in all): a chunk of one entry; chunks that are all
one bucket; chunks whose every entry opens a bucket; a run over three chunks whose middle chunk is head and tail partial at
once; the doubling and the cancelling branch right after an opener and on an accumulator with ZZ != 1, inside a chunk and
across a chunk end; identity bases; negative digits everywhere; bases that are no curve points, with every 30-bit limb of
both coordinates at or near its maximum (the corner operands of tests/field_model.py).  The streams of curve points are also
checked against the integer sum of their buckets."""
import ctypes
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import field_model as fm  # noqa: E402
from tests import group_model as gm  # noqa: E402
from tests.models import bucket_stage_model as model  # noqa: E402

P = gm.P
MERGE = 1                                   # what msm_enqueue picks for G1
ACC_INLINE, ACC_REFERENCE = 0, 1            # msm_accumulate_kernel<FpOps, false> / <FpOps, true> (xyzz_madd)
SCALARS = [0, 1, 2, 3, 5, 7, 11, 13, 200]   # base i = SCALARS[i] * generator; base 0 is the identity record
# canonical words with every 30-bit limb at or near 0x3fffffff, alternating 32-bit limbs, p - 1: coordinates of the corner
# bases (no curve points: the addition is plain arithmetic on them, the same in both kernels)
CORNER_WORDS = fm._limb_patterns(P) + fm.high_limb_values(P, 9, "accumulate inline") + [P - 1, 1, gm.ONE]
CORNER_BASES = [(x, y) for i, x in enumerate(CORNER_WORDS) for y in (CORNER_WORDS[i], CORNER_WORDS[(i + 5) % len(CORNER_WORDS)])]
FIRST_CORNER = len(SCALARS)
SHAPES = [(10, 8), (10, 52), (13, 8), (13, 52)]


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load().test


@pytest.fixture(scope="module")
def shape(lib):
    out = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(ACC_INLINE, MERGE, out) == 0
    ref = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(ACC_REFERENCE, MERGE, ref) == 0
    assert list(out) == list(ref)
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def bases():
    recs = [gm.affine_record(1, model.point(1, k)) for k in SCALARS] + CORNER_BASES
    assert all(v < P for r in recs for v in r)
    return gm._pack(recs)


# ----------------------------------------------------------------------------------------------------------------- streams
def _openers(first_digit, count, rnd):
    return [(first_digit + i, rnd.randrange(2), rnd.randrange(1, len(SCALARS))) for i in range(count)]


def _pad(entries, K, nb, rnd):
    """openers up to a multiple of K, so that the effective chunk is K itself"""
    d = entries[-1][0]
    fill = -len(entries) % K
    assert d + fill <= nb
    return entries + _openers(d + 1, fill, rnd)


def one_entry(K, nb, rnd):
    return [[(3, 1, 2)]]


def one_bucket(K, nb, rnd):
    """three chunks, one bucket (the last of the window): the middle chunk is all one bucket, head and tail partial"""
    return [[(nb, rnd.randrange(2), rnd.randrange(len(SCALARS))) for _ in range(3 * K)]]


def all_openers(K, nb, rnd):
    return [_openers(1, 2 * K - 1, rnd) + [(nb, 1, 4)]]


def three_chunks(K, nb, rnd):
    """K - 2 openers, then a run of 2 + K + 3 entries: tail partial of chunk 0, all of chunk 1, head partial of chunk 2"""
    e = _openers(1, K - 2, rnd)
    e += [(K, rnd.randrange(2), rnd.randrange(len(SCALARS))) for _ in range(2 + K + 3)]
    return [_pad(e, K, nb, rnd)]


def _branch_buckets(d):
    """(digit, sign, base) lists; with SCALARS = [0, 1, 2, 3, 5, 7, 11, 13, 200]"""
    G, G2, G3, G5, G7, G11, G13 = 1, 2, 3, 4, 5, 6, 7
    return [
        [(d, 1, G), (d, 1, G)],                                          # doubling right after the opener (ZZ = 1)
        [(d + 1, 0, G), (d + 1, 0, G2), (d + 1, 0, G3), (d + 1, 1, G5)],   # G + 2G, then + 3G: doubling with ZZ != 1
        [(d + 2, 0, G), (d + 2, 1, G), (d + 2, 1, G7), (d + 2, 1, G7)],    # P, -P: identity; then a copy, then a doubling
        [(d + 3, 1, G), (d + 3, 1, G2), (d + 3, 0, G3), (d + 3, 0, 0), (d + 3, 0, G11)],   # cancelling with ZZ != 1, identity base
        [(d + 4, 0, 0), (d + 4, 1, G13), (d + 4, 0, G13)],               # identity base first; the bucket ends as the identity
    ]


def branches(K, nb, rnd):
    """the branch buckets from the start of a chunk, and once more shifted so that they lie across chunk ends"""
    e = [x for b in _branch_buckets(1) for x in b]
    e = _pad(e, K, nb, rnd)
    e += _openers(e[-1][0] + 1, K - 3, rnd)
    e += [x for b in _branch_buckets(e[-1][0] + 1) for x in b]
    return [_pad(e, K, nb, rnd)]


def corners(K, nb, rnd):
    """buckets of one to seven corner bases of either sign, every corner base used"""
    e, d, k = [], 0, 0
    while k < 3 * len(CORNER_BASES):
        d += 1
        for _ in range(1 + d % 7):
            e.append((d, rnd.randrange(2), FIRST_CORNER + k % len(CORNER_BASES)))
            k += 1
    return [_pad(e, K, nb, rnd)]


def mixed(K, nb, rnd):
    """two windows with different z: skewed random buckets, curve points and identities"""
    out = []
    for _ in range(2):
        e = []
        for d in sorted(rnd.sample(range(1, nb + 1), 12)):
            count = rnd.randrange(1, 4) if rnd.randrange(3) else rnd.randrange(4, 2 * K)
            e += [(d, rnd.randrange(2), rnd.randrange(len(SCALARS))) for _ in range(count)]
        out.append(e)
    return out


STREAMS = [one_entry, one_bucket, all_openers, three_chunks, branches, corners, mixed]
ON_CURVE = {one_entry, one_bucket, all_openers, three_chunks, branches, mixed}


def build(stream, c, K):
    rnd = random.Random("accumulate inline %s %d %d" % (stream.__name__, c, K))
    lives = stream(K, 1 << (c - 1), rnd)
    n = max(len(e) for e in lives) + (5 if len(lives) > 1 else 0)
    windows, zstart = [], []
    for live in lives:
        z = n - len(live)
        windows.append([(live[0][0], rnd.randrange(2), rnd.randrange(len(SCALARS))) for _ in range(z)] + live)
        zstart.append(z)
    return dict(W=len(lives), n=n, c=c, K=K, cpw=(n + K - 1) // K, windows=windows, zstart=zstart)


def views(s, w=0):
    """the chunk views of window w, as the kernel computes them"""
    win, z = s["windows"][w], s["zstart"][w]
    Ke = model.effective_chunk(s["n"], z, s["cpw"], s["K"])
    digits = [d for d, _, _ in win]
    return Ke, [model.chunk_view(digits, s["n"], z, lane, Ke) for lane in range(s["cpw"])]


# ------------------------------------------------------------------------------------------------------------------- runs
def run(lib, worker, acc, s, bases, shape):
    rec, arec, guard, sentinel = shape[0], shape[1], shape[7], shape[11]
    W, n, c, cpw = s["W"], s["n"], s["c"], s["cpw"]
    pairs = np.array([(d << 32) | (sign << 31) | idx for win in s["windows"] for d, sign, idx in win], dtype=np.uint64)
    z = np.array(s["zstart"], dtype=np.uint32)
    plan_words = np.zeros(8, dtype=np.uint32)
    assert bases.shape[1] == arec
    args = [worker.ctx, acc, MERGE, gm._ptr(pairs), gm._ptr(z), W, n, gm._ptr(bases), bases.shape[0], arec, c, s["K"], cpw, None,
            gm._ptr(plan_words)]
    assert lib.bh_test_bucket_stage_dev(*(args + [None] * 7)) == 0
    plan = [int(v) for v in plan_words]
    sizes = dict(pts=(W << (c - 1)) * rec, head=W * cpw * rec, tail=W * cpw * rec, long=plan[5] * shape[8], big=plan[6] * shape[9],
                 pieces=plan[7] * rec, err=shape[10])
    bufs = {k: np.zeros(v + guard, dtype=np.uint8) for k, v in sizes.items()}
    assert lib.bh_test_bucket_stage_dev(*(args + [gm._ptr(bufs[k]) for k in ("pts", "head", "tail", "long", "big", "pieces", "err")])) == 0
    for k, v in sizes.items():
        assert (bufs[k][v:] == sentinel).all(), "bytes behind %s were written" % k
        bufs[k] = bufs[k][:v]
    return bufs


def counters(bufs):
    eof, ident, ident_top, nlong, nbig, npieces, madds, zeros = struct.unpack("<6I2Q", bufs["err"].tobytes()[:40])
    return dict(eof=eof, ident=ident, ident_top=ident_top, nlong=nlong, nbig=nbig, npieces=npieces, madds=madds, zeros=zeros)


def first_difference(a, b, rec):
    rows = np.nonzero((a.reshape(-1, rec) != b.reshape(-1, rec)).any(axis=1))[0]
    return rows[:8]


@pytest.mark.parametrize("c,K", SHAPES, ids=["c%d-K%d" % s for s in SHAPES])
@pytest.mark.parametrize("stream", STREAMS, ids=[f.__name__ for f in STREAMS])
def test_accumulation_stores_the_words_of_xyzz_madd(lib, worker, shape, bases, stream, c, K):
    s = build(stream, c, K)
    rec = shape[0]
    got = run(lib, worker, ACC_INLINE, s, bases, shape)
    ref = run(lib, worker, ACC_REFERENCE, s, bases, shape)
    for kind in ("head", "tail", "pts"):
        assert np.array_equal(got[kind], ref[kind]), "%s records %s differ from xyzz_madd's" % (kind, first_difference(got[kind], ref[kind], rec))
    cg, cr = counters(got), counters(ref)
    print(stream.__name__, c, K, "n %d chunks %d" % (s["n"], s["cpw"]), cg)
    assert cg == cr and cg["eof"] == 0 and cg["ident_top"] == 0
    # the additions the stream is meant to execute were executed: every live entry that neither opens a partial nor is an identity
    live = sum(s["n"] - z for z in s["zstart"])
    assert cg["madds"] <= live and (cg["madds"] > 0) == (stream not in (one_entry, all_openers))
    if stream in ON_CURVE:
        nb = 1 << (c - 1)
        rows = got["pts"].reshape(-1, rec)
        for w, (win, z) in enumerate(zip(s["windows"], s["zstart"])):
            want = model.brute_buckets(win, z, SCALARS)
            for d in range(1, nb + 1):
                row = rows[w * nb + d - 1]
                if d not in want:
                    assert not row.any(), ("empty bucket", w, d)
                    continue
                r = gm._unpack(row, 1)[0]
                assert all(v < 2 * P for v in r)
                assert gm.decode(1, r) == model.point(1, want[d]), ("bucket", w, d)


def test_streams_have_the_named_shapes():
    """the chunk layouts the cases are named after, by the kernel's own chunk arithmetic (host only)"""
    for c, K in SHAPES:
        nb = 1 << (c - 1)
        s = build(one_entry, c, K)
        assert s["n"] == 1 and views(s)[1][0][:2] == (0, 1)
        s = build(one_bucket, c, K)
        Ke, v = views(s)
        assert Ke == K and len(v) == 3 and v[1][4] and v[1][5] and v[0][5] and v[2][4] and v[1][2] == v[1][3] == nb
        s = build(all_openers, c, K)
        Ke, v = views(s)
        digits = [d for d, _, _ in s["windows"][0]]
        assert Ke == K and len(set(digits)) == len(digits) == 2 * K and not any(x[4] or x[5] for x in v)
        s = build(three_chunks, c, K)
        Ke, v = views(s)
        assert Ke == K and v[0][5] and not v[0][4] and v[1][4] and v[1][5] and v[1][2] == v[1][3] and v[2][4] and not v[2][5]
        s = build(branches, c, K)
        Ke, v = views(s)
        assert Ke == K and any(x[4] for x in v)            # the second copy of the branch buckets lies across chunk ends
        assert any(sign for win in s["windows"] for _, sign, _ in win)
        s = build(corners, c, K)
        used = {idx for _, _, idx in s["windows"][0]}
        assert set(range(FIRST_CORNER, FIRST_CORNER + len(CORNER_BASES))) <= used
        s = build(mixed, c, K)
        assert s["W"] == 2 and all(z > 0 for z in s["zstart"]) and s["zstart"][0] != s["zstart"][1]
    assert sum(build(f, c, K)["n"] * build(f, c, K)["W"] for f in STREAMS for c, K in SHAPES) < 8000
    for v in fm._limb_patterns(P)[:1] + fm.high_limb_values(P, 9, "accumulate inline"):
        limbs = [(v >> (30 * i)) & 0x3FFFFFFF for i in range(12)]
        assert all(l >= 0x3FFFFFFF - 255 for l in limbs)     # every full limb below the top one at or near its maximum


def test_one_addition_on_maximal_limbs(lib, worker):
    """bh_test_g1_madd_sliced_dev: accumulators whose four coordinates, and bases whose two, have every 30-bit limb at or
    near its maximum (lazily reduced below 2p / canonical below p), crossed; xyzz_madd's record next to the inline sliced one"""
    acc_words = fm._limb_patterns(2 * P) + fm.HIGH_LAZY[:13]
    q_words = fm._limb_patterns(P) + fm.high_limb_values(P, 5, "accumulate inline q")
    a_recs, q_recs = [], []
    for i, va in enumerate(acc_words):
        for j, vq in enumerate(q_words):
            other = acc_words[(i + 3) % len(acc_words)]
            a_recs.append((va, other, acc_words[(i + j) % len(acc_words)], va))
            q_recs.append((vq, q_words[(j + 1 + i) % len(q_words)]))
    a = np.ascontiguousarray(gm._pack(a_recs))
    q = np.ascontiguousarray(gm._pack(q_recs))
    n, rbytes = a.shape
    raw = np.zeros(2 * n * rbytes + gm.GUARD, dtype=np.uint8)
    raw[2 * n * rbytes:] = 0xA5
    flags = np.full(n + gm.GUARD // 4, 0xA5A5A5A5, dtype=np.uint32)
    dev = []
    try:
        for arr in (a, q, raw, flags):
            d = worker.alloc(arr.nbytes)
            dev.append(d)
            worker.upload(d, arr)
        assert lib.bh_test_g1_madd_sliced_dev(worker.ctx, dev[2], dev[3], dev[0], dev[1], n) == 0
        worker.download(raw, dev[2])
        worker.download(flags, dev[3])
    finally:
        for d in dev:
            worker.free(d)
    assert (raw[2 * n * rbytes:] == 0xA5).all() and (flags[n:] == 0xA5A5A5A5).all(), "bytes behind the results were written"
    res = raw[:2 * n * rbytes].reshape(2 * n, rbytes)
    bad = np.nonzero((res[:n] != res[n:]).any(axis=1))[0]
    assert bad.size == 0, "the inline sliced addition differs from xyzz_madd at cases %s" % bad[:8]
    assert ((flags[:n] & 1) == ((flags[:n] >> 1) & 1)).all() and (flags[:n] & 1).all()   # every case is an addition
