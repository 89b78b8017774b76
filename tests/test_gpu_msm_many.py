"""Several scalar vectors over ONE base vector in one job (bh_msm_many_*, bellman_amd.multiexp_many), on the GPU.  The
oracle is cref.multiexp(group, bases, skip, density, scalars_v) per vector: every record limb for limb, every return code.
Three ways each: the default dispatch, the many-plan forced (MANY_FORCE: the table flavour - Bases builds window tables
at these sizes), and its classic flavour (MANY_FORCE | NO_TABLE)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import scalar_mixes  # noqa: E402

Q = bls.Q
K_MAX = 16


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def _ways():
    from bellman_amd.multiexp import MANY_FORCE, NO_TABLE

    return (("default", 0), ("table", MANY_FORCE), ("classic", MANY_FORCE | NO_TABLE))


def _scalars(n, seed, special=True):
    """the scalars of test_gpu_parity (restated)"""
    sc = cref.random_fr(n, seed)
    if special and n >= 12:
        sc[1] = 0
        sc[2] = cref.ints_to_arr([1], 4)[0]
        sc[3] = cref.ints_to_arr([Q - 1], 4)[0]
        sc[4] = cref.ints_to_arr([1 << 200], 4)[0]
        sc[5] = sc[6]
        sc[7] = cref.ints_to_arr([2], 4)[0]
    return sc


_CASES = {}


def _case(group, n):
    """bases, K_MAX seeded vectors and the oracle's record for each: computed once per (group, n), never modified"""
    key = (group, n)
    if key not in _CASES:
        bases = cref.gen_bases(group, n, a=3, b=5)
        if n >= 12:
            bases[9] = bases[8]  # duplicate base
        vecs = np.stack([_scalars(n, 1000 * v + 50 + n) for v in range(K_MAX)])
        wants = []
        for v in range(K_MAX):
            rc, want = cref.multiexp(group, bases, 0, None, vecs[v])
            assert rc == 0
            wants.append(want)
        _CASES[key] = (bases, vecs, wants)
    return _CASES[key]


_BASES = {}


def _registered(worker, group, n):
    import bellman_amd

    key = (id(worker), group, n)
    if key not in _BASES:
        _BASES[key] = bellman_amd.Bases(worker, group, _case(group, n)[0])
    return _BASES[key]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("group,n", [(g, n) for g in (1, 2) for n in (1, 8, 9, 33, 100, 1000, 4113) if g == 1 or n <= 1000])
def test_many_matches_oracle(worker, group, n, k):
    import bellman_amd

    _, vecs, wants = _case(group, n)
    hb = _registered(worker, group, n)
    for name, flags in _ways():
        got = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), vecs[:k], flags=flags).wait()
        assert len(got) == k
        for v in range(k):
            assert isinstance(got[v], np.ndarray) and np.array_equal(got[v], wants[v]), (name, v)


@pytest.mark.parametrize("n", [33, 1000])
@pytest.mark.parametrize("group", [1, 2])
def test_many_special_vectors(worker, group, n):
    """an all-zero vector, an all-ones vector, a vector equal to another, a 90 %-boolean vector among ordinary ones"""
    import bellman_amd

    bases, vecs, wants = _case(group, n)
    hb = _registered(worker, group, n)
    zero = np.zeros((n, 4), dtype=np.uint64)
    ones = scalar_mixes.scalars("ones", n, 1)
    bool90 = scalar_mixes.scalars("bool90", n, 7)
    stack = np.stack([vecs[0], zero, ones, vecs[0], bool90, vecs[1]])
    expect = [wants[0], np.zeros_like(wants[0]), cref.multiexp(group, bases, 0, None, ones)[1], wants[0],
              cref.multiexp(group, bases, 0, None, bool90)[1], wants[1]]
    for name, flags in _ways():
        got = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), stack, flags=flags).wait()
        for v in range(len(stack)):
            assert np.array_equal(got[v], expect[v]), (name, v)


@pytest.mark.parametrize("group", [1, 2])
def test_many_density_skip_and_montgomery_scalars(worker, group):
    """n = 3000, 55 % dense, skip = 7, scalars as Rust `Scalar`s, k = 3, both flavours"""
    import bellman_amd

    n, k = 3000, 3
    rnd = np.random.default_rng(3)
    bits = rnd.random(n) < 0.55
    bases = cref.gen_bases(group, int(bits.sum()) + 7, a=2, b=7)
    hb = bellman_amd.Bases(worker, group, bases)
    dt = bellman_amd.DensityTracker(bits)
    vecs = np.stack([_scalars(n, 91 + v) for v in range(k)])
    wants = [cref.multiexp(group, bases, 7, cref.density_bitmap(bits), vecs[v]) for v in range(k)]
    mont = np.stack([cref.fr_to_mont(vecs[v]) for v in range(k)])
    for name, flags in _ways():
        got = bellman_amd.multiexp_many(worker, hb, dt, mont, skip=7, mont=True, flags=flags).wait()
        for v in range(k):
            assert wants[v][0] == 0 and np.array_equal(got[v], wants[v][1]), (name, v)
        got = bellman_amd.multiexp_many(worker, hb, dt, vecs, skip=7, flags=flags).wait()
        for v in range(k):
            assert np.array_equal(got[v], wants[v][1]), (name, v)


@pytest.mark.parametrize("group", [1, 2])
def test_many_strided_device_vectors(worker, group):
    """stride_bytes = 32 n + 64 through the _dev entry, a sentinel in the gap: the results do not change"""
    import bellman_amd

    n, k = 1000, 3
    _, vecs, wants = _case(group, n)
    hb = _registered(worker, group, n)
    stride = 32 * n + 64
    raw = np.full((k, stride), 0xA5, dtype=np.uint8)
    for v in range(k):
        raw[v, : 32 * n] = vecs[v].view(np.uint8).reshape(-1)
    d = worker.alloc(raw.nbytes)
    try:
        worker.upload(d, raw)
        for name, flags in _ways():
            got = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), None, scalars_dev=d, stride=stride, n=n, k=k,
                                            flags=flags).wait()
            for v in range(k):
                assert np.array_equal(got[v], wants[v]), (name, v)
        with pytest.raises(AssertionError):   # a stride shorter than a vector, or no multiple of 32
            bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), None, scalars_dev=d, stride=32 * n - 32, n=n, k=k)
        with pytest.raises(AssertionError):
            bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), None, scalars_dev=d, stride=32 * n + 8, n=n, k=k)
    finally:
        worker.free(d)


def _codes(items):
    from bellman_amd import UnexpectedEof, UnexpectedIdentity

    return [1 if isinstance(x, UnexpectedIdentity) else 2 if isinstance(x, UnexpectedEof) else 0 for x in items]


def test_many_error_semantics(worker):
    """The bases and scalars of test_msm_error_semantics with k = 3, the many-plan forced (both flavours).  The device
    flags are per job, so a job that meets an error answers every vector by the single-vector path: each code is the
    oracle's, and the vectors without an error still get their record.  (Vector 2 is random with a zero scalar at the
    identity base: a non-zero one there is an UnexpectedIdentity of its own.)"""
    import bellman_amd
    from bellman_amd.multiexp import HOLD, MANY_FORCE, NO_TABLE

    n = 200
    bases = cref.gen_bases(1, n, a=4, b=9)
    sc = cref.random_fr(n, 8)
    sc[:, 3] |= np.uint64(1 << 60)  # top-window digit non-zero for every scalar
    b2 = bases.copy()
    b2[17] = 0
    s2 = sc.copy()
    s2[17] = 0
    s3 = sc.copy()
    s3[17] = cref.ints_to_arr([5], 4)[0]  # identity only met in window 0
    rnd = cref.random_fr(n, 9)
    rnd[17] = 0

    def run(bs, vectors, flags):
        hb = bellman_amd.Bases(worker, 1, bs)
        got = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), np.stack(vectors), flags=flags).wait()
        want = [cref.multiexp(1, bs, 0, None, v) for v in vectors]
        assert _codes(got) == [w[0] for w in want]
        for g, w in zip(got, want):
            if w[0] == 0:
                assert np.array_equal(g, w[1])
        return _codes(got)

    for flags in (MANY_FORCE, MANY_FORCE | NO_TABLE):
        assert run(b2, [sc, s2, rnd], flags) == [1, 0, 0]
        assert run(b2[:-1], [sc, s3, s2], flags) == [1, 2, 2]     # bases one short: identity where the top window meets it first
        assert run(bases[:-1], [sc, s2, rnd], flags) == [2, 2, 2]
        assert run(bases, [sc, s2, rnd], flags) == [0, 0, 0]
        with pytest.raises(AssertionError):  # density length mismatch panics in the reference
            hb = bellman_amd.Bases(worker, 1, bases)
            bellman_amd.multiexp_many(worker, hb, bellman_amd.DensityTracker([True] * (n - 1)), np.stack([sc, s2]), flags=flags)
        with pytest.raises(AssertionError):  # a held many-job does not exist
            bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), np.stack([sc, s2]), flags=flags | HOLD)


def test_many_empty_shapes(worker):
    import bellman_amd
    from bellman_amd.multiexp import MANY_FORCE

    hb = _registered(worker, 1, 33)
    assert bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), np.zeros((0, 33, 4), dtype=np.uint64)).wait() == []
    got = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), np.zeros((3, 0, 4), dtype=np.uint64), flags=MANY_FORCE).wait()
    assert len(got) == 3 and not any(g.any() for g in got)


def test_many_jobs_in_flight_under_a_job_cap():
    """four many-jobs (k = 4, n = 1000) and four ordinary jobs in flight on one context whose cap is three"""
    import bellman_amd
    from bellman_amd.multiexp import MANY_FORCE, NO_TABLE

    w = bellman_amd.Worker(0)
    try:
        w.set_limits(max_jobs_in_flight=3)
        n, k = 1000, 4
        bases, vecs, wants = _case(1, n)
        hb = bellman_amd.Bases(w, 1, bases)
        jobs = []
        for j in range(4):
            sel = [(j + t) % K_MAX for t in range(k)]
            jobs.append(("many", sel, bellman_amd.multiexp_many(w, hb, bellman_amd.FullDensity(), vecs[sel],
                                                                 flags=MANY_FORCE | (NO_TABLE if j & 1 else 0))))
            jobs.append(("one", [j + 8], bellman_amd.multiexp(w, hb, bellman_amd.FullDensity(), vecs[j + 8])))
        for kind, sel, job in jobs:
            got = job.wait()
            got = got if kind == "many" else [got]
            for g, v in zip(got, sel):
                assert np.array_equal(g, wants[v]), (kind, v)
        assert w.info()["jobs_in_flight"] == 0
    finally:
        w.close()


@pytest.mark.parametrize("flavour", ["table", "classic"])
def test_many_stats(worker, flavour):
    """what the job executed: k times the sorted entries of the single job, one bucket set per vector (table flavour) or
    ceil(256 / c) per vector (classic)"""
    import bellman_amd
    from bellman_amd.multiexp import MANY_FORCE, NO_SMALL_PATH, NO_TABLE

    n, k = 1000, 5
    _, vecs, wants = _case(1, n)
    hb = _registered(worker, 1, n)
    extra = NO_TABLE if flavour == "classic" else 0
    _, _, one = bellman_amd.multiexp(worker, hb, bellman_amd.FullDensity(), vecs[0], flags=extra | NO_SMALL_PATH, stats=True).wait()
    got, ms, st = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), vecs[:k], flags=MANY_FORCE | extra, stats=True).wait()
    for v in range(k):
        assert np.array_equal(got[v], wants[v])
    assert st["sorted_entries"] == k * one["sorted_entries"]
    assert st["window_bits"] == one["window_bits"] and st["digit_columns"] == one["digit_columns"]
    assert st["bucket_sets"] == k * one["bucket_sets"]
    assert st["bucket_sets"] == (k if flavour == "table" else k * one["digit_columns"])
    # bh_msm_many_plan_info for ONE vector is the plan the single job ran: c, K, passes' worth of entries
    from bellman_amd import _lib

    out = (ctypes.c_uint * 12)()
    assert _lib.load().bh_msm_many_plan_info(n, 1, 1, one["window_bits"] if flavour == "table" else 0, worker.info()["num_cus"], out) == 0
    assert (out[0], out[3], out[1] * out[6]) == (one["window_bits"], one["chunk"], one["sorted_entries"])
    assert ms[0] > 0 and ms[0] >= ms[2]


# ---- the digit and sort stage on its own, against the Python model ------------------------------------------------------
_MODEL = {}


def _stage_model(nd, k, c, dense):
    """scalars, density, and the model's pairs in the classic flavour (base_stride = 0): once per shape"""
    import random

    from tests.models import many_digits_model as mdm

    key = (nd, k, c, dense)
    if key not in _MODEL:
        rnd = random.Random(1000 * nd + 10 * k + c + dense)
        vs = [[rnd.randrange(mdm.Q) for _ in range(nd)] for _ in range(k)]
        vs[0][1], vs[0][2], vs[0][3], vs[1][4] = 0, 1, mdm.Q - 1, 1 << 200
        density = [rnd.random() < 0.55 for _ in range(nd)] if dense else None
        skip = 7
        # with a density map the last two dense entries run off the end of the bases (EOF); without one nothing does
        n_bases = skip + (sum(density) - 2 if dense else nd)
        pairs, eof = mdm.many_pairs(vs, c, density, skip, n_bases, 0)
        sc = np.stack([cref.ints_to_arr(v, 4) for v in vs])
        _MODEL[key] = (sc, density, skip, n_bases, np.array(pairs, dtype=np.uint64), eof)
    return _MODEL[key]


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("c", [8, 13])
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("nd", [70, 4097])
def test_many_stage_against_model(worker, nd, k, c, table, dense):
    """bh_test_many_stage_dev: the shipped msm_run_stages under a many-plan, in buffers of production's exact sizes with
    guards behind them, against tests/models/many_digits_model.py - the multiset of pairs in every bucket set (and their
    order by digit), zstart per set, ErrFlags.eof, and the guards intact."""
    from bellman_amd import _lib
    from tests.models import many_digits_model as mdm

    lib = _lib.load()
    sc, density, skip, n_bases, classic_pairs, eof = _stage_model(nd, k, c, dense)
    wd = (256 + c - 1) // c
    stride = 5000 if table else 0
    pairs = classic_pairs.copy()
    if table:   # digit column j addresses table row j
        j = (np.arange(pairs.size, dtype=np.uint64) // np.uint64(nd)) % np.uint64(wd)
        pairs = (pairs & ~np.uint64(0x7FFFFFFF)) | ((pairs + j * np.uint64(stride)) & np.uint64(0x7FFFFFFF))
    words = bellman_amd_words(density)
    W = k if table else k * wd
    n_set = wd * nd if table else nd
    got = np.zeros(W * n_set, dtype=np.uint64)
    zstart = np.zeros(W, dtype=np.uint32)
    err = np.zeros(16, dtype=np.uint32)
    plan, guards = np.zeros(4, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.bh_test_many_stage_dev(worker.ctx, int(table), c, p(sc), 0, nd, k, None if words is None else p(words), skip, n_bases,
                                    stride, p(got), p(zstart), p(err), p(plan), p(guards))
    assert rc == 0
    assert list(plan) == [W, n_set, (c + 7) // 8, wd]
    assert guards.all(), guards
    assert bool(err[0]) == eof and eof == dense          # ErrFlags.eof
    assert err[1] == 0                                   # nothing consumes a base in these stages
    want_sets = pairs.reshape(W, n_set)
    got_sets = got.reshape(W, n_set)
    assert np.array_equal(np.sort(got_sets, axis=1), np.sort(want_sets, axis=1))
    digits = got_sets >> np.uint64(32)
    assert (np.diff(digits.astype(np.int64), axis=1) >= 0).all()        # every set sorted by |digit|
    assert list(zstart) == mdm.zero_counts([list(map(int, s)) for s in want_sets])


def bellman_amd_words(density):
    import bellman_amd

    return None if density is None else bellman_amd.DensityTracker(density).words()


# ---- the dispatch rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,many", [(1024, 4, True), (1024, 16, True), (1024, 3, False), (1024, 17, False), (1024, 40, False),
                                      (1000, 8, False)])
def test_many_default_dispatch(worker, n, k, many):
    """without MANY_FORCE the many-plan is taken inside the measured box only (4 <= k <= 16, 2^10 ... 2^18 scalars, bases
    with their window table); outside it - more vectors included - the call issues ordinary jobs: the job's statistics
    show which ran, and every record is the oracle's either way"""
    import bellman_amd

    bases = cref.gen_bases(1, n, a=3, b=5)
    hb = bellman_amd.Bases(worker, 1, bases)
    assert hb.table_info()[0] != 0
    vecs = np.stack([_scalars(n, 7000 + v % 3) for v in range(k)])
    wants = [cref.multiexp(1, bases, 0, None, vecs[v])[1] for v in range(3)]
    got, _, st = bellman_amd.multiexp_many(worker, hb, bellman_amd.FullDensity(), vecs, stats=True).wait()
    for v in range(k):
        assert np.array_equal(got[v], wants[v % 3]), v
    assert st["bucket_sets"] == (k if many else 1)
    hb.release()
