"""Checking a powers-of-tau transcript on the GPU: bh_bases_validate, the coefficient expander, the eight sums,
bh_pairing_product_is_one and bh_powers_of_tau_verify.  Transcripts are built on the device from uploaded exponents
(bh_fixed_base_mul_dev), so the exponents are arbitrary and the exponent model (tests/models/ptau_verify_model.py) predicts
every mask and every sum exactly: all comparisons are equalities, there are no tolerances."""

import ctypes
import functools
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import compressed_model as cm  # noqa: E402
from tests import pointgen  # noqa: E402
from tests.models import pairing_stage_model as psm  # noqa: E402
from tests.models import ptau_verify_model as model  # noqa: E402
from tests.test_compressed_cpu import header_constants  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401

P, Q = bls.P, bls.Q
LENGTHS = [(2, 2), (3, 2), (9, 9), (10, 10), (17, 9), (130, 65)]
SEED_A, SEED_B = bytes(range(1, 33)), bytes((11 * i + 3) % 256 for i in range(32))
GEN = {1: cref.g1_generator(), 2: cref.g2_generator()}
WORDS = {1: 12, 2: 24}
PT_RANGE, PT_IS_INF, PT_OFF_CURVE, PT_NOT_IN_SUBGROUP = 4, 16, 32, 64
INVALID_POINT, POINT_AT_INFINITY = 6, 7


def _lib_ctx(worker):
    from bellman_amd import _lib

    return _lib.load(), worker.ctx


def _points(worker, group, exps):
    """[x]G for every exponent as affine records, computed on the device (x = 0: the identity record)"""
    from bellman_amd.errors import check

    lib, ctx = _lib_ctx(worker)
    n, rec = len(exps), WORDS[group] * 8
    sc = np.frombuffer(b"".join((x % Q).to_bytes(32, "little") for x in exps), dtype=np.uint64).copy()
    out = np.zeros((n, WORDS[group]), dtype=np.uint64)
    d_sc, d_pts = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bh_dev_alloc(ctx, n * 32, ctypes.byref(d_sc)))
    check(lib.bh_dev_alloc(ctx, n * rec, ctypes.byref(d_pts)))
    try:
        check(lib.bh_dev_upload(ctx, d_sc, sc.ctypes.data_as(ctypes.c_void_p), n * 32))
        check(lib.bh_fixed_base_mul_dev(ctx, group, GEN[group].ctypes.data_as(ctypes.c_void_p), d_sc, n, 0, d_pts, None))
        check(lib.bh_dev_download(ctx, out.ctypes.data_as(ctypes.c_void_p), d_pts, n * rec))
    finally:
        lib.bh_dev_free(ctx, d_sc)
        lib.bh_dev_free(ctx, d_pts)
    for i, x in enumerate(exps):
        if x % Q == 0:
            out[i] = 0
    return out


class _Device:
    """a model transcript as four registered handles and the beta_g2 record"""

    def __init__(self, worker, tr, patch=None):
        from bellman_amd.multiexp import Bases

        recs = [_points(worker, 2 if v == 1 else 1, x) for v, x in enumerate(tr.vec)]
        self.beta_g2 = _points(worker, 2, [tr.beta2])[0]
        if patch:
            patch(recs, self)
        self.bases = [Bases(worker, 2 if v == 1 else 1, r) for v, r in enumerate(recs)]

    def args(self):
        return (*self.bases, self.beta_g2)


def _verify(worker, dev, seed, validate_points=False):
    """(return code, failed, bad_vector, bad_index) of bh_powers_of_tau_verify"""
    from bellman_amd.ceremony import PtauReport, _PowersOfTau

    lib, ctx = _lib_ctx(worker)
    t = _PowersOfTau(*[b._h for b in dev.bases], dev.beta_g2.ctypes.data)
    rep = PtauReport()
    rc = lib.bh_powers_of_tau_verify(ctx, ctypes.byref(t), seed, 1 if validate_points else 0, ctypes.byref(rep))
    return rc, rep.failed, rep.bad_vector, rep.bad_index


def _expect(mask):
    return (0 if mask == 0 else 10), mask


def _toxic(tag):
    rnd = random.Random("ptau verify %s" % (tag,))
    return rnd.randrange(2, Q), rnd.randrange(1, Q), rnd.randrange(1, Q)


# ---- coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 129])
def test_device_expander_equals_hashlib(worker, count):
    lib, ctx = _lib_ctx(worker)
    for v, seed in ((0, SEED_A), (1, SEED_B), (2, SEED_A), (3, SEED_B)):
        out = np.zeros(count * 32, dtype=np.uint8)
        assert lib.bh_test_ptau_rlc_dev(ctx, seed, v, count, out.ctypes.data_as(ctypes.c_void_p)) == 0
        assert out.tobytes() == model.coefficient_bytes(seed, v, count)


# ---- the eight sums ----------------------------------------------------------------------------------------------------
def _sums(worker, dev, seed):
    from bellman_amd.ceremony import _PowersOfTau

    lib, ctx = _lib_ctx(worker)
    t = _PowersOfTau(*[b._h for b in dev.bases], dev.beta_g2.ctypes.data)
    out = np.zeros((8, 24), dtype=np.uint64)
    rcs = (ctypes.c_int * 8)()
    assert lib.bh_test_ptau_sums(ctx, ctypes.byref(t), seed, out.ctypes.data_as(ctypes.c_void_p), rcs) == 0
    return out, list(rcs)


@pytest.mark.parametrize("n1,n", LENGTHS)
def test_sums_equal_the_oracle(worker, n1, n):
    """arbitrary exponents (no relation between the points): P(V) = [sum rho_i x_i]G, Q(V) = [sum rho_i x_{i+1}]G"""
    rnd = random.Random(1000 * n1 + n)
    tr = model.Transcript(*[[rnd.randrange(1, Q) for _ in range(k)] for k in (n1, n, n, n)], rnd.randrange(1, Q))
    dev = _Device(worker, tr)
    got, rcs = _sums(worker, dev, SEED_A)
    assert rcs == [0] * 8
    for v, (p, q, ident) in enumerate(model.sums(tr, SEED_A)):
        group = 2 if v == 1 else 1
        assert not ident
        for k, e in ((2 * v, p), (2 * v + 1, q)):
            assert got[k, :WORDS[group]].tobytes() == cref.point_mul(group, GEN[group], e).tobytes(), (v, k)
    other, _ = _sums(worker, dev, SEED_B)
    assert all(other[k].tobytes() != got[k].tobytes() for k in range(8))   # another seed: other sums


# ---- verdicts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n", LENGTHS)
def test_consistent_transcript_passes(worker, n1, n):
    tr = model.Transcript.consistent(*_toxic((n1, n)), n1, n)
    dev = _Device(worker, tr)
    for seed in (SEED_A, SEED_B):
        assert model.mask(tr, seed) == 0
        assert _verify(worker, dev, seed)[:2] == (0, 0)
    assert _verify(worker, dev, SEED_A, validate_points=True) == (0, 0, 0, 0)


def test_one_point_alpha_and_beta_vectors_pass(worker):
    tr = model.Transcript.consistent(*_toxic("one"), 3, 2)
    tr.vec[2], tr.vec[3] = tr.vec[2][:1], tr.vec[3][:1]
    assert model.mask(tr, SEED_A) == 0
    assert _verify(worker, _Device(worker, tr), SEED_A, validate_points=True) == (0, 0, 0, 0)
    tr.beta2 += 1   # ... and the one equation that still reads B fails alone
    tr = tr.copy()
    assert _verify(worker, _Device(worker, tr), SEED_A)[:2] == (10, model.BETA_G2)


N1, N = 17, 9


def _faults():
    out = []
    for v in range(4):
        ln = N1 if v == 0 else N
        for where, idx in (("first", 0), ("second", 1), ("middle", ln // 2), ("last", ln - 1)):
            out.append(("vec%d-%s" % (v, where), ("exponent", v, idx)))
        out.append(("vec%d-identity-inside" % v, ("zero", v, ln // 2)))
    out += [("tau-g2-differs", ("tau_g2",)), ("foreign-beta-g2", ("beta_g2",)), ("b-scaled-alone", ("scale_b", False)),
            ("b-and-beta-g2-scaled", ("scale_b", True)), ("tau-zero", ("tau_zero",))]
    return out


def _apply(tr, fault):
    kind = fault[0]
    if kind == "exponent":
        tr.vec[fault[1]][fault[2]] += 1
    elif kind == "zero":
        tr.vec[fault[1]][fault[2]] = 0
    elif kind == "tau_g2":
        tr.vec[1] = [pow(0xABCDEF, i, Q) for i in range(len(tr.vec[1]))]
    elif kind == "beta_g2":
        tr.beta2 = 0x5EED
    elif kind == "scale_b":
        tr.vec[3] = [3 * x for x in tr.vec[3]]
        if fault[1]:
            tr.beta2 *= 3
    elif kind == "tau_zero":   # tau = 0: every power from index 1 onwards is the identity
        tr.vec = [[x if i == 0 else 0 for i, x in enumerate(v)] for v in tr.vec]
    return tr.copy()


@pytest.mark.parametrize("name,fault", _faults(), ids=[f[0] for f in _faults()])
def test_one_fault_gives_the_models_mask(worker, name, fault):
    tr = _apply(model.Transcript.consistent(*_toxic("faults"), N1, N), fault)
    dev = _Device(worker, tr)
    want = model.mask(tr, SEED_A)
    assert (want == 0) == (name == "b-and-beta-g2-scaled")
    assert _verify(worker, dev, SEED_A)[:2] == _expect(want)
    # another seed: other coefficients, the same verdict
    assert model.mask(tr, SEED_B) == want
    assert _verify(worker, dev, SEED_B)[:2] == _expect(want)


@pytest.mark.parametrize("head", ["g1", "s1", "g2", "s2", "a0", "b0", "beta_g2"])
def test_identity_head_sets_only_head(worker, head):
    tr = model.Transcript.consistent(*_toxic("head"), 10, 10)

    def patch(recs, dev):
        v, i = {"g1": (0, 0), "s1": (0, 1), "g2": (1, 0), "s2": (1, 1), "a0": (2, 0), "b0": (3, 0), "beta_g2": (None, 0)}[head]
        if v is None:
            dev.beta_g2[:] = 0
        else:
            recs[v][i] = 0

    dev = _Device(worker, tr, patch)
    assert _verify(worker, dev, SEED_A)[:2] == (10, model.HEAD)


def test_off_curve_head_sets_only_head(worker):
    tr = model.Transcript.consistent(*_toxic("head2"), 3, 2)

    def patch(recs, dev):
        recs[1][1] = cref.g2_from_py(psm.g2_points()["off_curve"])[0]

    assert _verify(worker, _Device(worker, tr, patch), SEED_A)[:2] == (10, model.HEAD)


def test_short_vectors_and_wrong_groups_are_invalid_arguments(worker):
    tr = model.Transcript.consistent(*_toxic("short"), 3, 2)
    good = _Device(worker, tr)
    short = model.Transcript.consistent(*_toxic("short"), 3, 2)
    short.vec[0] = short.vec[0][:1]
    assert _verify(worker, _Device(worker, short), SEED_A)[0] == -2
    good.bases[0], good.bases[1] = good.bases[1], good.bases[0]
    assert _verify(worker, good, SEED_A)[0] == -2


# ---- validation of resident points ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _classes(group):
    """kind -> one python point"""
    if group == 1:
        return {"off_subgroup": pointgen.g1_on_curve_not_in_subgroup(5), "order3": psm.g1_points()["order3"][0],
                "order3_neg": psm.g1_points()["order3"][1], "off_curve": psm.g1_points()["off_curve"][1], "identity": None}
    g2 = psm.g2_points()
    return {"off_subgroup": pointgen.g2_on_curve_not_in_subgroup(5), "special": g2["off_subgroup"][0],
            "off_curve": g2["off_curve"][0], "identity": None}


@functools.lru_cache(maxsize=None)   # (the tables repeat a handful of points; the model costs 0.25 s per point)
def _model_status(group, pt):
    beta, cx, cy = header_constants()
    curve = bls.G1 if group == 1 else bls.G2
    if pt is None:
        return PT_IS_INF
    if not curve.on_curve(pt):
        return PT_OFF_CURVE
    ok = cm.g1_endo_in_subgroup(pt, beta) if group == 1 else cm.g2_endo_in_subgroup(pt, cx, cy)
    assert ok == (curve.mul(pt, Q) is None)   # the endomorphism predicate is the subgroup test
    return 0 if ok else PT_NOT_IN_SUBGROUP


def _first_bad(status, forbid_identity):
    for i, s in enumerate(status):
        if s & ~PT_IS_INF:
            return INVALID_POINT, i
        if s and forbid_identity:
            return POINT_AT_INFINITY, i
    return 0, 0


def _validate(worker, bases, first, count, flags):
    lib, ctx = _lib_ctx(worker)
    st = np.full(count + 1, 0xDEAD, dtype=np.uint32)
    bad = ctypes.c_size_t(0)
    rc = lib.bh_bases_validate(ctx, bases._h, first, count, flags, st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bad))
    assert st[count] == 0xDEAD
    return rc, bad.value, [int(s) for s in st[:count]]


def _reader(worker, group, pts, flags):
    """(return code, bad index) of bh_bases_read_uncompressed - the [q] P path - on the same points"""
    lib, ctx = _lib_ctx(worker)
    enc = bls.g1_uncompressed if group == 1 else bls.g2_uncompressed
    buf = np.frombuffer(b"".join(enc(p) for p in pts), dtype=np.uint8)
    h, bad = ctypes.c_void_p(), ctypes.c_size_t(0)
    rc = lib.bh_bases_read_uncompressed(ctx, group, buf.ctypes.data_as(ctypes.c_void_p), len(pts), flags, ctypes.byref(h), ctypes.byref(bad))
    if rc == 0:
        lib.bh_bases_release(ctx, h)
    return rc, bad.value if rc else 0


@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("group", [1, 2])
def test_validate_equals_model_and_reader(worker, group, n):
    from bellman_amd.multiexp import Bases

    curve = bls.G1 if group == 1 else bls.G2
    rnd = random.Random(100 * group)   # the same five subgroup points at every n: the model's verdicts are cached
    good = [curve.mul(curve.gen, rnd.randrange(1, Q)) for _ in range(min(n, 5))]
    base = [good[i % len(good)] for i in range(n)]
    from_py = cref.g1_from_py if group == 1 else cref.g2_from_py
    positions = sorted({p for p in (0, 63, 64, n - 1) if p < n})
    kinds = _classes(group)
    tables = [[(p, k)] for k in kinds for p in positions]                                    # one bad point at one position
    tables.append([(p, list(kinds)[i % len(kinds)]) for i, p in enumerate(positions)])       # several kinds at once
    tables.append([(p, list(kinds)[-1 - i % len(kinds)]) for i, p in enumerate(positions)])  # ... the identity first
    tables.append([])                                                                        # all good
    for placed in tables:
        pts = list(base)
        for p, k in placed:
            pts[p] = kinds[k]
        want = [_model_status(group, pt) for pt in pts]
        bases = Bases(worker, group, from_py(pts))
        for flags in (3, 1, 2, 0):   # CHECKED | FORBID_IDENTITY, CHECKED, FORBID_IDENTITY, none
            exp_status = want if flags & 1 else [s & PT_IS_INF for s in want]
            rc, bad, status = _validate(worker, bases, 0, n, flags)
            assert status == exp_status, (placed, flags)
            assert (rc, bad if rc else 0) == _first_bad(exp_status, flags & 2), (placed, flags)
            if flags & 1:
                assert (rc, bad if rc else 0) == _reader(worker, group, pts, flags), (placed, flags)
        bases.release()


def test_validate_sub_ranges_and_wrapped_handle(worker):
    from bellman_amd.errors import check
    from bellman_amd.multiexp import Bases

    lib, ctx = _lib_ctx(worker)
    for group in (1, 2):
        curve = bls.G1 if group == 1 else bls.G2
        kinds = _classes(group)
        pts = [curve.mul(curve.gen, 3 + i % 4) for i in range(130)]
        pts[63], pts[64], pts[129] = kinds["off_subgroup"], None, kinds["off_curve"]
        recs = (cref.g1_from_py if group == 1 else cref.g2_from_py)(pts)
        owned = Bases(worker, group, recs)
        dev = ctypes.c_void_p()
        check(lib.bh_dev_alloc(ctx, recs.nbytes, ctypes.byref(dev)))
        check(lib.bh_dev_upload(ctx, dev, recs.ctypes.data_as(ctypes.c_void_p), recs.nbytes))
        wrapped = Bases.wrap_device(worker, group, dev, 130)
        for b in (owned, wrapped):
            assert _validate(worker, b, 0, 63, 3)[:2] == (0, 0)
            assert _validate(worker, b, 60, 10, 3) == (INVALID_POINT, 3, [0, 0, 0, PT_NOT_IN_SUBGROUP, PT_IS_INF, 0, 0, 0, 0, 0])
            assert _validate(worker, b, 64, 66, 3)[:2] == (POINT_AT_INFINITY, 0)
            assert _validate(worker, b, 64, 66, 1)[:2] == (INVALID_POINT, 65)
            assert _validate(worker, b, 65, 64, 3)[:2] == (0, 0)
            assert _validate(worker, b, 130, 0, 3)[:2] == (0, 0)
            assert _validate(worker, b, 100, 31, 3)[0] == -2 and _validate(worker, b, 131, 0, 3)[0] == -2
        # the Python method: raises with the index, returns the status words
        with pytest.raises(IOError) as e:
            owned.validate(first=60, count=10)
        assert e.value.index == 3
        assert list(owned.validate(first=64, count=2, return_status=True)) == [PT_IS_INF, 0]
        wrapped.release()
        owned.release()
        lib.bh_dev_free(ctx, dev)


def test_non_canonical_coordinate_is_invalid(worker):
    from bellman_amd.multiexp import Bases

    recs = cref.g1_from_py([bls.G1.gen, bls.G1.gen])
    x = cref.limbs_to_int([int(w) for w in recs[1, :6]]) + P   # the same residue, not the canonical value
    recs[1, :6] = cref.int_to_limbs(x, 6)
    assert _validate(worker, Bases(worker, 1, recs), 0, 2, 1) == (INVALID_POINT, 1, [0, PT_RANGE])


@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_validate_points_flag_reports_vector_and_index(worker, v):
    import bellman_amd
    from bellman_amd.ceremony import verify_powers_of_tau

    tr = model.Transcript.consistent(*_toxic("points"), 10, 10)
    group = 2 if v == 1 else 1
    from_py = cref.g1_from_py if group == 1 else cref.g2_from_py
    for kind, code, exc in (("off_subgroup", INVALID_POINT, bellman_amd.InvalidPoint), ("identity", POINT_AT_INFINITY, bellman_amd.PointAtInfinity)):
        def patch(recs, dev):
            recs[v][5] = from_py([_classes(group)[kind]])[0]

        dev = _Device(worker, tr, patch)
        assert _verify(worker, dev, SEED_A, validate_points=True) == (code, model.POINTS, v, 5)
        with pytest.raises(exc) as e:
            verify_powers_of_tau(worker, *dev.args(), seed=SEED_A)
        assert (e.value.report.failed, e.value.report.bad_vector, e.value.report.bad_index) == (model.POINTS, v, 5)


def test_python_wrapper_verdicts(worker):
    import bellman_amd
    from bellman_amd.ceremony import verify_powers_of_tau

    tr = model.Transcript.consistent(*_toxic("py"), 9, 9)
    assert verify_powers_of_tau(worker, *_Device(worker, tr).args()).failed == 0   # a seed from the CSPRNG
    tr.vec[2][4] += 1
    tr = tr.copy()
    with pytest.raises(bellman_amd.InvalidTranscript) as e:
        verify_powers_of_tau(worker, *_Device(worker, tr).args(), seed=SEED_A)
    assert e.value.report.failed == model.mask(tr, SEED_A) == model.ALPHA


# ---- pairing product -----------------------------------------------------------------------------------------------------
def _pairs(a, b):
    return (np.array([cref.point_mul(1, GEN[1], x) if x % Q else np.zeros(12, np.uint64) for x in a]),
            np.array([cref.point_mul(2, GEN[2], x) if x % Q else np.zeros(24, np.uint64) for x in b]))


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_pairing_product_against_exponents(worker, n):
    from bellman_amd.ceremony import pairing_product_is_one

    rnd = random.Random(n)
    a = [rnd.randrange(1, Q) for _ in range(n)]
    b = [rnd.randrange(1, Q) for _ in range(n)]
    if n > 1:   # sum a_i b_i = 0
        b[-1] = -sum(x * y for x, y in zip(a[:-1], b[:-1])) * pow(a[-1], -1, Q) % Q
        assert sum(x * y for x, y in zip(a, b)) % Q == 0
        assert pairing_product_is_one(worker, *_pairs(a, b)) is True
        b[0] = (b[0] + 1) % Q
    assert sum(x * y for x, y in zip(a, b)) % Q != 0
    assert pairing_product_is_one(worker, *_pairs(a, b)) is False
    # an identity on either side contributes 1
    for side in (0, 1):
        aa, bb = list(a), list(b)
        (aa if side == 0 else bb)[0] = 0
        want = sum(x * y for x, y in zip(aa, bb)) % Q == 0
        assert want == (n == 1)
        assert pairing_product_is_one(worker, *_pairs(aa, bb)) is want


def test_pairing_product_edges(worker):
    import bellman_amd
    from bellman_amd.ceremony import pairing_product_is_one

    lib, ctx = _lib_ctx(worker)
    assert pairing_product_is_one(worker, np.zeros((0, 12), np.uint64), np.zeros((0, 24), np.uint64)) is True
    p, q = _pairs([3, 5], [7, 11])
    for side in (0, 1):
        pp, qq = p.copy(), q.copy()
        if side == 0:
            pp[1] = cref.g1_from_py(psm.g1_points()["off_curve"][1:])[0]
        else:
            qq[1] = cref.g2_from_py(psm.g2_points()["off_curve"])[0]
        with pytest.raises(bellman_amd.InvalidPoint):
            pairing_product_is_one(worker, pp, qq)
    one = ctypes.c_int(7)
    assert lib.bh_pairing_product_is_one(ctx, p.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p), 16385, ctypes.byref(one)) == -2


# ---- concurrency -----------------------------------------------------------------------------------------------------------
def test_four_threads_verify_four_transcripts(worker):
    trs = []
    for k in range(4):
        tr = model.Transcript.consistent(*_toxic("thread %d" % k), 130 if k % 2 else 17, 65 if k % 2 else 9)
        if k >= 2:
            tr.vec[k][3] += 1
            tr = tr.copy()
        trs.append(tr)
    devs = [_Device(worker, tr) for tr in trs]
    alone = [_verify(worker, d, SEED_A, validate_points=True) for d in devs]
    assert [r[:2] for r in alone] == [_expect(model.mask(tr, SEED_A)) for tr in trs]
    assert [r[1] for r in alone] == [0, 0, model.ALPHA, model.BETA]
    got = [None] * 4

    def run(k):
        got[k] = [_verify(worker, devs[k], SEED_A, validate_points=True) for _ in range(3)]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == [[r] * 3 for r in alone]


def test_validate_across_chunks(worker):
    """2^20 + 65 G1 records: the call walks them in chunks of 2^20, and the bad records sit behind the first chunk, so
    bad_index, the status words and the early exit all go through the second chunk's offset"""
    from bellman_amd.errors import check
    from bellman_amd.groth16 import fr_to_mont_array
    from bellman_amd.multiexp import Bases

    lib, ctx = _lib_ctx(worker)
    chunk, n = 1 << 20, (1 << 20) + 65
    sc, pts = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bh_dev_alloc(ctx, n * 32, ctypes.byref(sc)))
    check(lib.bh_dev_alloc(ctx, n * 96, ctypes.byref(pts)))
    try:
        gs = fr_to_mont_array([0x1234567, 1])
        check(lib.bh_fr_powers_dev(ctx, sc, n, gs[0:1].ctypes.data_as(ctypes.c_void_p), gs[1:2].ctypes.data_as(ctypes.c_void_p), None))
        check(lib.bh_fixed_base_mul_dev(ctx, 1, GEN[1].ctypes.data_as(ctypes.c_void_p), sc, n, 1, pts, None))
        kinds = _classes(1)
        placed = {chunk: "identity", chunk + 5: "off_curve", chunk + 64: "off_subgroup"}
        for idx, kind in placed.items():
            rec = cref.g1_from_py([kinds[kind]])
            check(lib.bh_dev_upload(ctx, ctypes.c_void_p(pts.value + idx * 96), rec.ctypes.data_as(ctypes.c_void_p), 96))
        bases = Bases.wrap_device(worker, 1, pts, n)
        want = np.zeros(n, dtype=np.uint32)
        for idx, kind in placed.items():
            want[idx] = _model_status(1, kinds[kind])
        assert [int(want[i]) for i in placed] == [PT_IS_INF, PT_OFF_CURVE, PT_NOT_IN_SUBGROUP]

        def run(first, count, flags, with_status=True):
            st = np.full(count + 1, 0xDEAD, dtype=np.uint32)
            bad = ctypes.c_size_t(0)
            rc = lib.bh_bases_validate(ctx, bases._h, first, count, flags, st.ctypes.data_as(ctypes.c_void_p) if with_status else None,
                                       ctypes.byref(bad))
            assert st[count] == 0xDEAD
            return rc, bad.value, st[:count]

        for first in (0, 7):   # first = 7: the chunk boundary falls at record 2^20 + 7
            for flags, code, where in ((3, POINT_AT_INFINITY, chunk), (1, INVALID_POINT, chunk + 5)):
                rc, bad, st = run(first, n - first, flags)
                assert (rc, bad) == (code, where - first), (first, flags)
                assert np.array_equal(st, want[first:]), (first, flags)
                assert run(first, n - first, flags, with_status=False)[:2] == (code, where - first)
        rc, bad, st = run(chunk + 6, 59, 3)   # a range inside the second chunk
        assert (rc, bad) == (INVALID_POINT, 58) and np.array_equal(st, want[chunk + 6:])
        assert run(0, chunk, 3)[:2] == (0, 0)
        bases.release()
    finally:
        lib.bh_dev_free(ctx, sc)
        lib.bh_dev_free(ctx, pts)
