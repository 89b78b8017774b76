"""Stage 4 of a multiexp on its own (run with `pytest -m gpu` on a MI355X): msm_accumulate_kernel, msm_merge_chunks_kernel and
the tail kernels over sorted streams built for the index arithmetic (tests/models/bucket_stage_streams.py), launched by the
functions msm_enqueue launches them with (bh_test_bucket_stage_dev), in every accumulate instantiation and every merge
combination msm_enqueue can reach, and - per merge form - with every admissible number G of workers per medium run.

Everything the kernels write is compared with tests/models/bucket_stage_model.py: every bucket (gm.decode, which asserts
ZZ^3 = ZZZ^2; an untouched bucket must be all-zero bytes), every head and tail slot (the unwritten ones still hold the
sentinel the hook filled them with), the piece results, both queues as sets of records, the piece ranges (disjoint, covering
[0, npieces)), the six counters, and the guard bytes behind every buffer.  Points are compared for equality: integer work,
no tolerance.  Record sizes, the piece length, the workers per wavefront and the range of G come from
bh_test_bucket_stage_shape."""
import ctypes
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import group_model as gm  # noqa: E402
from tests.models import bucket_stage_model as model  # noqa: E402
from tests.models import bucket_stage_streams as streams  # noqa: E402

ACC_FORMS = {0: "g1-reg", 1: "g1-lds", 2: "g2-lds", 3: "g2-reg", 4: "g2-triples", 5: "g2-pairs"}
MERGE_FORMS = {0: "g1-xyzz", 1: "g1-k2", 2: "k3-xyzz", 3: "k3-k6", 4: "g2-fused", 5: "g2-split"}
GROUP = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 5: 2}     # of an accumulate form and of a merge form alike
DEFAULT_MERGE = {1: 1, 2: 3}                     # what msm_enqueue picks for a group when nothing is forced
ACC_OF = {0: 0, 1: 0, 2: 4, 3: 4, 4: 2, 5: 2}    # the accumulate form a merge form's cases run behind
SMALL_SET = {5}


def cases():
    """(accumulate form, merge form, stream, base stride (0: dense), every admissible G?)"""
    out = [(ACC_OF[m], m, name, 0, True) for m in MERGE_FORMS for name in streams.STREAM_NAMES]
    for a in ACC_FORMS:
        m = DEFAULT_MERGE[GROUP[a]]
        out += [(a, m, name, 0, False) for name in ("boundaries", "branches") if a != ACC_OF[m]]
    out.append((0, DEFAULT_MERGE[1], "boundaries", 128, False))
    return out


def case_id(case):
    a, m, name, stride, every_g = case
    return "%s+%s-%s%s" % (ACC_FORMS[a], MERGE_FORMS[m], name, "-stride%d" % stride if stride else "")


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


PLAN_FIELDS = ("walk", "run_lanes", "runs_on_pairs", "big_chunks", "piece", "max_long", "max_big", "max_pieces")
_bases = {}


def bases(g, stride, arec):
    """the pool as affine records `stride` bytes apart"""
    if (g, stride) not in _bases:
        raw = np.zeros((len(streams.POOL), stride), dtype=np.uint8)
        raw[:, :arec] = gm._pack([gm.affine_record(g, model.point(g, k)) for k in streams.POOL])
        _bases[(g, stride)] = raw
    return _bases[(g, stride)]


def run(lib, worker, acc, merge, s, stride, G, shape):
    """-> (plan, dict of the returned buffers without their guards)"""
    g = GROUP[acc]
    rec, arec, guard, sentinel = shape[0], shape[1], shape[7], shape[11]
    W, n, c, cpw = s["W"], s["n"], s["c"], s["chunks_per_window"]
    pairs = np.array([(d << 32) | (sign << 31) | idx for win in s["windows"] for d, sign, idx in win], dtype=np.uint64)
    z = np.array(s["zstart"], dtype=np.uint32)
    ov = list(s["overrides"])
    ov[1] = G
    ov = np.array(ov, dtype=np.uint32)
    b = bases(g, stride or arec, arec)
    plan_words = np.zeros(8, dtype=np.uint32)
    args = [worker.ctx, acc, merge, gm._ptr(pairs), gm._ptr(z), W, n, gm._ptr(b), len(streams.POOL), stride or arec, c, s["K"], cpw,
            gm._ptr(ov), gm._ptr(plan_words)]
    assert lib.bh_test_bucket_stage_dev(*(args + [None] * 7)) == 0
    plan = dict(zip(PLAN_FIELDS, (int(v) for v in plan_words)))
    sizes = dict(pts=(W << (c - 1)) * rec, head=W * cpw * rec, tail=W * cpw * rec, long=plan["max_long"] * shape[8],
                 big=plan["max_big"] * shape[9], pieces=plan["max_pieces"] * rec, err=shape[10])
    bufs = {k: np.zeros(v + guard, dtype=np.uint8) for k, v in sizes.items()}
    assert lib.bh_test_bucket_stage_dev(*(args + [gm._ptr(bufs[k]) for k in ("pts", "head", "tail", "long", "big", "pieces", "err")])) == 0
    for k, v in sizes.items():
        assert (bufs[k][v:] == sentinel).all(), "bytes behind %s were written" % k
        bufs[k] = bufs[k][:v]
    return plan, bufs


def records(g, raw, rec):
    return raw.reshape(-1, rec)


def as_point(g, row):
    r = gm._unpack(row, 1)[0]
    assert all(v < 2 * gm.P for v in r)
    return gm.decode(g, r)


def check(g, s, plan, bufs, shape, tag, slots_like=None):
    rec, sentinel = shape[0], shape[11]
    m = model.stage(s["windows"], s["zstart"], s["scalars"], s["K"], s["chunks_per_window"], plan["walk"], plan["big_chunks"],
                    plan["piece"])
    W, c, cpw = s["W"], s["c"], s["chunks_per_window"]
    nb = 1 << (c - 1)
    # the counters
    eof, ident, ident_top, nlong, nbig, npieces, madds, zeros = struct.unpack("<6I2Q", bufs["err"].tobytes()[:40])
    print(tag, "nlong %d nbig %d npieces %d ident %d madds %d zeros %d" % (nlong, nbig, npieces, ident, madds, zeros), plan)
    assert (eof, ident_top) == (0, 0), tag
    assert (nlong, nbig, npieces, ident, madds, zeros) == (m["nlong"], m["nbig"], m["npieces"], m["ident"], m["madds"], m["zeros"]), tag
    assert nlong <= plan["max_long"] and nbig <= plan["max_big"] and npieces <= plan["max_pieces"], tag
    # both queues, as sets of records; what lies behind them is untouched
    lq = np.frombuffer(bufs["long"].tobytes(), dtype=np.uint32).reshape(-1, 4)
    assert {tuple(int(v) for v in r) for r in lq[:nlong]} == m["long_runs"], tag
    assert (bufs["long"][nlong * shape[8]:] == sentinel).all(), tag
    bq = np.frombuffer(bufs["big"].tobytes(), dtype=np.uint32).reshape(-1, 8)
    big = [tuple(int(v) for v in r) for r in bq[:nbig]]
    assert {(r[0], r[1], r[2], r[3], r[5], r[6]) for r in big} == m["big_runs"] and all(r[7] == 0 for r in big), tag
    assert (bufs["big"][nbig * shape[9]:] == sentinel).all(), tag
    covered = sorted(q for r in big for q in range(r[4], r[4] + r[5]))
    assert covered == list(range(npieces)), (tag, "piece ranges")
    # the piece results: written for runs of more than one piece only
    prow = records(g, bufs["pieces"], rec)
    written = set()
    for w_, lane, d, last, p0, np_, done, pad in big:
        if np_ > 1:
            for q, k in enumerate(model.piece_sums(m["windows"][w_], lane, last, np_, plan["piece"])):
                assert as_point(g, prow[p0 + q]) == model.point(g, k), (tag, "piece", w_, d, q)
                written.add(p0 + q)
    for q in range(len(prow)):
        assert q in written or (prow[q] == sentinel).all(), (tag, "piece slot", q)
    # head and tail slots (what the accumulation writes does not depend on the merge parameters: the same bytes as before)
    for kind in ("head", "tail"):
        rows = records(g, bufs[kind], rec)
        if slots_like is not None and (slots_like[kind] == bufs[kind]).all():
            continue
        for w_, win in enumerate(m["windows"]):
            for lane in range(cpw):
                row = rows[w_ * cpw + lane]
                if lane in win[kind]:
                    assert as_point(g, row) == model.point(g, win[kind][lane]), (tag, kind, w_, lane)
                else:
                    assert (row == sentinel).all(), (tag, kind, "unwritten slot", w_, lane)
    # every bucket
    rows = records(g, bufs["pts"], rec)
    for w_, win in enumerate(m["windows"]):
        for d in range(1, nb + 1):
            row = rows[w_ * nb + d - 1]
            if d in win["buckets"]:
                assert as_point(g, row) == model.point(g, win["buckets"][d]), (tag, "bucket", w_, d)
            else:
                assert not row.any(), (tag, "empty bucket", w_, d)


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_bucket_stage_against_the_index_model(worker, lib, case):
    acc, merge, name, stride, every_g = case
    out = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(acc, merge, out) == 0
    shape = [int(v) for v in out]
    s = streams.stream(name, shape[2], merge in SMALL_SET)
    widths = [0]
    if every_g:
        widths, G = [], shape[5]
        while G <= shape[6]:
            widths.append(G)
            G <<= 1
    first = None
    for G in widths:
        plan, bufs = run(lib, worker, acc, merge, s, stride, G, shape)
        assert plan["piece"] == shape[2] and (G == 0 or plan["run_lanes"] == G) and plan["runs_on_pairs"] == (merge & 1 if merge < 4 else 0)
        if s["overrides"][2]:
            assert (plan["walk"], plan["big_chunks"]) == (s["overrides"][0] or streams.WALK, s["overrides"][2])
        check(GROUP[acc], s, plan, bufs, shape, "%s G=%d" % (case_id(case), plan["run_lanes"]), first)
        first = first or bufs


def test_hook_refuses_streams_that_could_leave_the_buffers(worker, lib):
    """validated on the host, before any launch: nothing is written to the output buffers"""
    out = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(0, 1, out) == 0
    shape = [int(v) for v in out]
    W, n, c, K, cpw = 1, 64, 9, 8, 8
    good = [(1 + i // 5, i & 1, 1 + i % 3) for i in range(n)]
    b = bases(1, shape[1], shape[1])
    big = np.full(1 << 20, 0x5C, dtype=np.uint8)

    def rc(entries, z=0, n_bases=len(streams.POOL), stride=shape[1], n_=n, cpw_=cpw, acc=0):
        pairs = np.array([(d << 32) | (sign << 31) | idx for d, sign, idx in entries], dtype=np.uint64)
        zs = np.array([z], dtype=np.uint32)
        plan_words = np.zeros(8, dtype=np.uint32)
        r = lib.bh_test_bucket_stage_dev(worker.ctx, acc, 1, gm._ptr(pairs), gm._ptr(zs), W, n_, gm._ptr(b), n_bases, stride, c, K, cpw_,
                                         None, gm._ptr(plan_words), *([gm._ptr(big)] * 7))
        assert r == 0 or (big == 0x5C).all()
        return r

    bad_order = list(good)
    bad_order[40] = (1, 0, 1)
    assert rc(bad_order) != 0                                              # a digit that decreases
    assert rc([(0, 0, 1)] + good[1:]) != 0                                 # digit 0 among the live entries
    assert rc(good[:-1] + [((1 << (c - 1)) + 1, 0, 1)]) != 0               # digit beyond the last bucket
    assert rc(good[:10] + [(good[10][0], 0, len(streams.POOL))] + good[11:]) != 0   # base index past the vector
    assert rc(good, n_bases=3) != 0
    assert rc(good, z=n + 1) != 0
    assert rc(good, cpw_=7) != 0                                           # n > chunks_per_window K
    assert rc(good, stride=128, acc=1) != 0 and rc(good, stride=100) != 0  # strides no accumulate launch uses
    assert rc([(0, 0, 99)] * 7 + good[7:], z=7) == 0                       # anything may lie below z
