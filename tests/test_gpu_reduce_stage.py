"""Stage 5 of a multiexp on its own (run with `pytest -m gpu` on a MI355X): the row / column sums, their two-stage split, the
bit sums and totals over FILLED BUCKETS of the test's choice, issued by the function msm_enqueue issues them with
(launch_reduce, through bh_test_reduce_stage_dev) into buffers of exactly production's sizes, then the shipped host tail.

Buckets hold k G for |k| <= 8, picked from a pool of raw records - every point in several scalings with +p masks, the identity
all-zero and as ZZ = 0 with garbage - by a seeded index array, so every expected value is an integer sum
(tests/models/reduce_stage_model.py replays the launches bh_test_reduce_plan hands out) turned into a point once per output.  All
sums stay far below the group order: "sum = 0" is "identity".  Classes: dense, sparse (90 % all-zero records), every bucket the
same point (every tree level doubles), alternating +-P (level one cancels), one live bucket at either end of the first and
last window, all identities.  Shapes: the smallest that reach each path - see CASES; the plan query says what each reaches, and
test_cases_reach_every_path asserts the list of tests/test_reduce_stage_model_cpu.py over what ran here.

Before anything is launched the replay checks the case's own plan (bounds, written before read, written once): a wrong plan
does not reach the device.  Exact comparisons throughout: the guards, every coordinate < 2p, ZZ^3 = ZZZ^2 (gm.decode), every
record of bits and the affine result; rows, cols and part cell for cell up to 8192 cells a buffer, above that 1024 seeded
cells plus each window's first and last; cells the plan does not write still hold the sentinel."""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import group_model as gm  # noqa: E402
from tests.models import reduce_stage_model as rsm  # noqa: E402

G1, K3, G2 = 0, 1, 2
CLASSIC, TABLE = 0, 1
MAX_K, REPS = 8, 6
FULL_COMPARE, SAMPLE = 8192, 1024
OTHER_CLASSES = ("same_point", "alternating", "live_first_0", "live_first_top", "live_last_0", "live_last_top", "identities")


def _cases():
    """(form, kind, c, num_cus override (0: the context's own), bucket class)"""
    shapes = []
    # degenerate: lo_bits = 0 and no low bit sums at c = 2
    shapes += [(f, k, c, 0) for c in (2, 3, 4) for k in (CLASSIC, TABLE) for f in (G1, K3, G2)]
    # production's small sets
    small = [(TABLE, 8), (TABLE, 10), (TABLE, 13), (CLASSIC, 8), (CLASSIC, 13)]
    shapes += [(f, k, c, 0) for k, c in small for f in (G1, K3, G2)]
    # the edges of the two-stage rule: 2^16 buckets (no pieces), 2^17 (the smallest with), 19 x 2^13 with Lw = 64 (and Sr = 1 on
    # 32 compute units), 2^21 (the largest with pieces) and 2^22 (none again)
    # (one-lane G2 has no two-stage sums and no edge there; the shapes run for it too, as its sets of 2^16 ... 2^17 buckets)
    shapes += [(f, TABLE, c, 0) for c in (17, 18) for f in (G1, K3, G2)]
    shapes += [(f, CLASSIC, 14, n) for n in (0, 32) for f in (G1, K3)] + [(G2, CLASSIC, 14, 0)]
    shapes += [(G1, TABLE, 22, 0), (G1, TABLE, 23, 0)]
    # production's big sets: 16 windows of 2^15 (one-lane G2: the joint lane choice), the 2^15 and 2^19 buckets of a table
    shapes += [(G1, CLASSIC, 16, 0), (G2, CLASSIC, 16, 0), (G1, TABLE, 16, 0), (G1, TABLE, 20, 0), (K3, TABLE, 20, 0)]
    out = [s + (cls,) for s in shapes for cls in ("dense", "sparse")]
    out += [(f, k, c, 0, cls) for k, c in ((TABLE, 10), (TABLE, 18), (CLASSIC, 8)) for f in (G1, K3, G2) for cls in OTHER_CLASSES
            if not (k == TABLE and cls.startswith("live_last"))]   # (one window: the last is the first)
    # a partitioned chip
    out += [(f, k, c, n, "dense") for k, c in small for f in (G1, K3, G2) for n in (32, 64, 128)]
    out += [(f, TABLE, 18, n, "dense") for f in (G1, K3) for n in (32, 64, 128)]
    return out


CASES = _cases()


def case_id(case):
    form, kind, c, num_cus, cls = case
    return "%s-%s-c%d%s-%s" % (rsm.FORMS[form], rsm.KINDS[kind], c, "-cus%d" % num_cus if num_cus else "", cls)


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


# ------------------------------------------------------------------------------------------------------------ the buckets
_pools, _points = {}, {}


def pool(g):
    """raw records: row (k + MAX_K) * REPS + r is representation r of k G; k = 0: all-zero (r even) or ZZ = 0 with garbage"""
    if g not in _pools:
        import random

        rnd = random.Random("reduce stage pool %d" % g)
        lam = gm._lambda_source(g, "reduce stage")
        nmask = 4 * gm.FIELDS[g].width
        recs = []
        for k in range(-MAX_K, MAX_K + 1):
            for r in range(REPS):
                if k == 0:
                    recs.append(gm.identity_record(g, rnd if r % 2 else None))
                else:
                    recs.append(gm.represent(g, point(g, k), next(lam), rnd.randrange(1 << nmask) if r else 0))
        _pools[g] = gm._pack(recs)
    return _pools[g]


def point(g, k):
    """k G (None: the identity), every value computed once"""
    pts = _points.setdefault(g, {0: None, 1: gm.GEN[g]})
    if k not in pts:
        if k < 0:
            pts[k] = gm.neg(g, point(g, -k))
        elif k <= 1 << 12:
            for i in range(2, k + 1):
                if i not in pts:
                    pts[i] = gm.add(g, pts[i - 1], gm.GEN[g])
        else:
            pts[k] = gm.mul(g, gm.GEN[g], k)
    return pts[k]


def buckets_of(plan, cls, seed):
    """(k of every bucket, representation of every bucket)"""
    NB, nb, W = plan["NB"], plan["nb"], plan["W"]
    rng = np.random.default_rng([plan["c"], plan["kind"], plan["form"], seed])
    reps = rng.integers(0, REPS, size=NB, dtype=np.int64)
    if cls == "dense":
        ks = rng.integers(-MAX_K, MAX_K + 1, size=NB, dtype=np.int8)
    elif cls == "sparse":
        u = rng.random(NB)
        ks = np.where(u < 0.07, rng.integers(-MAX_K, MAX_K + 1, size=NB, dtype=np.int8), 0).astype(np.int8)
        reps = np.where((ks == 0) & (u < 0.97), 0, reps)     # 90 % all-zero records, 3 % identities with garbage, 7 % live
    elif cls == "same_point":
        ks = np.full(NB, 3, dtype=np.int8)
    elif cls == "alternating":
        ks = np.where(np.arange(NB) % 2 == 0, 5, -5).astype(np.int8)
    elif cls == "identities":
        ks = np.zeros(NB, dtype=np.int8)
    else:
        ks = np.zeros(NB, dtype=np.int8)
        reps[:] = 0
        w = 0 if "first" in cls else W - 1
        ks[w * nb + (0 if cls.endswith("_0") else nb - 1)] = 7
    return ks, (ks.astype(np.int64) + MAX_K) * REPS + reps


# -------------------------------------------------------------------------------------------------------------- the checks
TWO_P = [(2 * gm.P >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def below_2p(raw):
    """raw: (cells, record bytes) - every 48-byte coefficient below 2p"""
    v = np.ascontiguousarray(raw).view("<u8").reshape(raw.shape[0], raw.shape[1] // 48, 6)
    lt = np.zeros(v.shape[:2], dtype=bool)
    eq = np.ones(v.shape[:2], dtype=bool)
    for limb in range(5, -1, -1):
        lt |= eq & (v[:, :, limb] < np.uint64(TWO_P[limb]))
        eq &= v[:, :, limb] == np.uint64(TWO_P[limb])
    return bool(lt.all())


def compare_cells(g, raw, want, written, cells, tag, sentinel):
    for i in cells:
        if not written[i]:
            assert (raw[i] == sentinel).all(), (tag, "a cell the plan does not write was written", int(i))
            continue
        rec = gm._unpack(raw[i], 1)[0]
        assert gm.decode(g, rec) == point(g, int(want[i])), (tag, "cell", int(i), "holds another point than %d G" % int(want[i]))


def chosen_cells(n, windows, seed):
    if n <= FULL_COMPARE:
        return range(n)
    rng = np.random.default_rng([n, seed])
    edges = [w * (n // windows) + e for w in range(windows) for e in (0, n // windows - 1)]
    return sorted(set(edges) | set(int(x) for x in rng.integers(0, n, size=SAMPLE)))


def check_outputs(plan, cls, val, written, out, affine, total, tag):
    """what came back against the replay: out[buffer] = (cells, record bytes) raw, affine = the host tail's record"""
    g, c, sentinel = rsm.FORM_GROUP[plan["form"]], plan["c"], plan["sentinel"]
    # rows and cols (a window's rows, then cols behind all rows), part, bits
    W, H, Lw = plan["W"], 1 << plan["hi_bits"], 1 << plan["lo_bits"]
    for b in (rsm.ROWCOL, rsm.PART, rsm.BITS):
        n = rsm.sizes(plan)[b]
        raw, wr = out[b][:n], written[b] == 1
        assert below_2p(raw[wr]), (tag, rsm.BUF_NAMES[b], "a coordinate is not below 2p")
        assert (raw[~wr] == sentinel).all(), (tag, rsm.BUF_NAMES[b], "a cell the plan does not write was written")
        if b == rsm.ROWCOL:
            cells = sorted(set(chosen_cells(W * H, W, 1)) | set(W * H + i for i in chosen_cells(W * Lw, W, 2)))
        elif b == rsm.PART:
            # part = [W][H][Sr] row pieces, then [W][Lw][Sc] column pieces: each window's first and last cell of both
            two = plan["two_len"]
            nr = W * H * (Lw // min(two, Lw)) if n else 0
            cells = sorted(set(chosen_cells(nr, W, 3)) | set(nr + i for i in chosen_cells(n - nr, W, 4))) if n else []
        else:
            cells = range(n)
        compare_cells(g, raw, val[b], wr, cells, (tag, rsm.BUF_NAMES[b]), sentinel)
    # the host tail over the device's bits
    k = total % bls.Q
    want = gm.mul(g, gm.GEN[g], k) if k else None
    if cls == "identities":
        assert want is None
    if cls.startswith("live_"):
        w = 0 if "first" in cls else W - 1
        assert total == 7 * ((1 if cls.endswith("_0") else plan["nb"]) << (c * w)), tag
    assert gm._unpack(affine[:plan["affine"]], 1)[0] == gm.affine_record(g, want), (tag, "the affine result")


_reached = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reduce_stage_against_the_integer_model(worker, lib, case):
    form, kind, c, num_cus, cls = case
    g, tag = rsm.FORM_GROUP[form], case_id(case)
    t0 = time.time()
    plan, launches = rsm.query(lib, form, kind, c, num_cus, worker.ctx)
    rec, guard, sentinel = plan["record"], plan["guard"], plan["sentinel"]
    ks, idx = buckets_of(plan, cls, 11)
    try:   # a wrong plan must not reach the device
        val, written = rsm.execute(plan, launches, ks)
        rsm.check_written_once(plan, written)
    except rsm.PlanError as e:
        pytest.fail("%s: the plan fails the bounds check, nothing was launched: %s" % (tag, e))
    _reached[case[:4]] = rsm.coverage(plan, launches)
    rowcol_want, bits_want = rsm.definitions(plan, ks)
    assert np.array_equal(val[rsm.ROWCOL], rowcol_want) and np.array_equal(val[rsm.BITS], bits_want), tag
    total = rsm.tail(plan, bits_want)
    assert total == rsm.weighted(plan, ks), tag
    t1 = time.time()

    pts = pool(g)[idx]
    assert pts.shape == (plan["NB"], rec)
    out = {b: np.zeros((max(1, n), rec), dtype=np.uint8) for b, n in rsm.sizes(plan).items() if b != rsm.PTS}
    guards = np.zeros(4, dtype=np.uint32)
    affine = np.full(plan["affine"] + 64, 0xA5, dtype=np.uint8)
    rc = lib.bh_test_reduce_stage_dev(worker.ctx, form, kind, c, num_cus, gm._ptr(pts), gm._ptr(out[rsm.ROWCOL]), gm._ptr(out[rsm.PART]),
                                      gm._ptr(out[rsm.BITS]), gm._ptr(guards), gm._ptr(affine))
    t2 = time.time()
    assert rc == 0, (tag, rc)
    assert guards.tolist() == [1, 1, 1, 1], (tag, "guards (pts, rowcol, part, bits)", guards.tolist())
    assert (affine[plan["affine"]:] == 0xA5).all(), tag

    check_outputs(plan, cls, val, written, out, affine, total, tag)
    print("%s: NB %d, %d launches %s, model %.2f s, device call %.2f s, checks %.2f s" % (
        tag, plan["NB"], len(launches), [(l["kind"], l["waves"], l["blocks"]) for l in launches], t1 - t0, t2 - t1, time.time() - t2))


def test_cases_reach_every_path(worker, lib):
    """the list of tests/test_reduce_stage_model_cpu.py, over the cases of this module (queried again when run alone)"""
    for form in rsm.FORMS:
        facts = set()
        for case in CASES:
            if case[0] != form:
                continue
            if case[:4] not in _reached:
                _reached[case[:4]] = rsm.coverage(*rsm.query(lib, case[0], case[1], case[2], case[3], worker.ctx))
            facts |= _reached[case[:4]]
        want = {("worker", k, w) for k, w in rsm.WORKERS[form]}
        want |= {("want_part", False), ("t_from_cols", False), ("t_from_cols", True), ("lo_bits", 0)}
        if form in (G1, K3):   # (one-lane G2 has no two-stage sums, and Sc = 1 is out of reach: test_reduce_stage_model_cpu.py)
            want |= {("want_part", True), ("Sr>1", True), ("Sr>1", False), ("Sc>1", True)}
        assert want <= facts, (rsm.FORMS[form], sorted(want - facts, key=str))
