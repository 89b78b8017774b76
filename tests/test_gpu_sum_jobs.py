"""msm_sum_kernel<WK, NWAVES> on its own (run with `pytest -m gpu` on a MI355X): up to three SumDesc jobs in one launch through
sum_launch (bh_test_sum_jobs_dev), in every worker kind and workgroup width msm_enqueue launches - where a whole multiexp
reaches one of them or another depending on its size and on the number of compute units.

The expected outputs are the index model of tests/models/bucket_sum_model.py over tests/group_model.add; the device's raw
records are decoded (ZZ^3 = ZZZ^2 is asserted on the way) and compared as points, identities as identities.  The input
records are group_model representations - a random scaling, +p masks on the coordinates - of small multiples of the
generator of either sign (so that partial sums meet as equal points: a tree level doubles - and as opposite points: a level
gives the identity), of other subgroup points, and identities in the all-zero and the ZZ = 0-with-garbage form; every fifth
record repeats its neighbour in another scaling and every eleventh negates it.  The shapes are the smallest that reach
each path of the kernel:
  one lane per point (G1; G2 with its accumulators in LDS), 1 wavefront: G = 1, 4, 64 workers per output (strided), 1, 8 (bits)
  lane pairs, 1 wavefront: G = 1, 4, 32; 7 outputs, not a multiple of the 32 / G outputs of a workgroup
  lane pairs, 2 and 4 wavefronts: one output per workgroup, G = 64 and 128 over 160 elements (workers with two, one, no
    element) and over the 256 selected of 512
  lane triples, 4 wavefronts: G = 1, 16, 32, 64 (the wider two cross wavefronts through LDS); 100 outputs of one worker each,
    which is the 21-per-wavefront mapping and more than one 84-worker workgroup
  lane sextets, 4 wavefronts: G = 1, 8, 16, 32; 5 outputs
  three different jobs in one launch (lane pairs; lane triples with 84- and 64-worker workgroups side by side)
Bytes after the last output must come back untouched."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import group_model as gm  # noqa: E402
from tests.models import bucket_sum_model as bsm  # noqa: E402

N_IN = 704
STRIDED = dict(mode="strided", groups=7, count=12, inner=3, stride=3, istride=1, group_shift=6, splits=1)
BITS = dict(mode="bits", groups=8, count=16, inner=4, stride=1, istride=0, group_shift=4, splits=1)
WIDE_STRIDED = dict(mode="strided", groups=3, count=160, inner=1, stride=1, istride=0, group_shift=8, splits=1)
WIDE_BITS = dict(mode="bits", groups=9, count=512, inner=9, stride=1, istride=0, group_shift=9, splits=1)
SPLIT = dict(mode="strided", groups=100, count=16, inner=5, stride=1, istride=16, group_shift=7, splits=4)
FIVE = dict(groups=5)


def cases():
    """(form, wavefronts per workgroup, [(job, workers per output), ...])"""
    out = []
    for form in (0, 2):
        out += [(form, 1, [(STRIDED, G)]) for G in (1, 4, 64)] + [(form, 1, [(BITS, G)]) for G in (1, 8)]
    out += [(1, 1, [(job, G)]) for job in (STRIDED, BITS) for G in (1, 4, 32)]
    out += [(1, waves, [(job, 32 * waves)]) for waves in (2, 4) for job in (WIDE_STRIDED, WIDE_BITS)]
    out += [(3, 4, [(job, G)]) for job in (STRIDED, BITS) for G in (1, 16, 32, 64)] + [(3, 4, [(SPLIT, 1)])]
    out += [(5, 4, [(dict(job, **FIVE), G)]) for job in (STRIDED, BITS) for G in (1, 8, 16, 32)]
    out += [(1, 1, [(STRIDED, 4), (BITS, 32), (SPLIT, 1)]), (3, 4, [(STRIDED, 32), (SPLIT, 1), (BITS, 1)])]
    return out


def case_id(case):
    form, waves, jobs = case
    return "%s-w%d-%s" % (gm.FORMS[form], waves, "+".join("%s%dx%d-G%d" % (d["mode"][0], d["groups"], d["count"], G) for d, G in jobs))


_tables = {}


def table(g):
    """(the affine points, None = identity; their raw records) of group g, built once"""
    if g not in _tables:
        rnd = random.Random("sum jobs %d" % g)
        pool = gm.subgroup_points(g)
        lam = gm._lambda_source(g, "sum jobs")
        nmask = 4 * gm.FIELDS[g].width
        pts, recs = [], []
        for i in range(N_IN):
            if i % 5 == 1 and pts[-1] is not None:
                pt = pts[-1]
            elif i % 11 == 3 and pts[-1] is not None:
                pt = gm.neg(g, pts[-1])
            elif i % 9 == 4:
                pt = None
            else:
                pt = pool[rnd.randrange(3)] if rnd.randrange(3) else pool[rnd.randrange(len(pool))]
                pt = gm.neg(g, pt) if rnd.randrange(2) else pt
            pts.append(pt)
            if pt is None:
                recs.append(gm.identity_record(g, rnd if i % 2 else None))
            else:
                recs.append(gm.represent(g, pt, next(lam), rnd.randrange(1 << nmask) if i % 3 else 0))
        _tables[g] = (pts, recs)
    return _tables[g]


_want = {}


def expected(g, d):
    """the model's outputs of job d over the table of group g; shared by every case with that job (a sum does not depend on
    how many workers share it: tests/test_bucket_sum_model_cpu.py)"""
    key = (g, tuple(sorted(d.items())))
    if key not in _want:
        _want[key] = bsm.run_job(d, table(g)[0], 1, add=lambda a, b: gm.add(g, a, b), zero=None)
    return _want[key]


def job_words(d, G, out_off):
    return [1 if d["mode"] == "strided" else 2, d["groups"], d["count"], d["inner"], d["stride"], d["istride"], d["group_shift"],
            d["splits"], G, 0, out_off]


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
def inputs(worker):
    """the two tables in device memory, uploaded once"""
    dev = {}
    for g in (1, 2):
        arr = gm._pack(table(g)[1])
        dev[g] = worker.alloc(arr.nbytes)
        worker.upload(dev[g], arr)
    yield dev
    for d in dev.values():
        worker.free(d)


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_sum_jobs_against_the_index_model(worker, lib, inputs, case):
    form, waves, jobs = case
    g = gm.GROUP[form]
    rbytes = 4 * 48 * gm.FIELDS[g].width
    n_out = sum(d["groups"] for d, _ in jobs)
    words, off = [], 0
    for d, G in jobs:
        words += job_words(d, G, off)
        off += d["groups"]
    words = np.array(words, dtype=np.uint32)
    raw = np.full(n_out * rbytes + gm.GUARD, 0xA5, dtype=np.uint8)
    out = worker.alloc(raw.nbytes)
    try:
        worker.upload(out, raw)
        rc = lib.bh_test_sum_jobs_dev(worker.ctx, form, waves, inputs[g], N_IN, out, n_out, gm._ptr(words), len(jobs))
        assert rc == 0, case_id(case)
        worker.download(raw, out)
    finally:
        worker.free(out)
    assert (raw[n_out * rbytes:] == 0xA5).all(), "bytes after the %d outputs were written" % n_out
    got = gm._unpack(raw[:n_out * rbytes], n_out)
    off = 0
    for d, G in jobs:
        want = expected(g, d)
        assert len(want) == d["groups"]
        for k, pt in enumerate(want):
            rec = got[off + k]
            assert all(v < 2 * gm.P for v in rec), (case_id(case), k)
            assert gm.decode(g, rec) == pt, (case_id(case), d["mode"], k)
        off += d["groups"]
