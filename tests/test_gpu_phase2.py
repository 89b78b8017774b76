"""Checking a circuit-specific ceremony step on the GPU: bh_bases_first_difference, the four sums,
bh_groth16_params_verify_step, bh_pairing_same_ratio_each and the helpers of bellman_amd/ceremony.py.  Points are built in
the exponent ([x]G on the device), so the exponent model (tests/models/phase2_model.py) predicts every mask, vector, index,
sum and verdict exactly: all comparisons are equalities, there are no tolerances."""

import ctypes
import functools
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import pointgen  # noqa: E402
from tests.models import pairing_stage_model as psm  # noqa: E402
from tests.models import phase2_model as model  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401
from tests.test_gpu_ptau_verify import GEN, SEED_A, SEED_B, WORDS, _lib_ctx, _points  # noqa: E402

Q = bls.Q
INVALID_POINT, POINT_AT_INFINITY, INVALID_TRANSCRIPT = 6, 7, 10
NH, NL, NA = 65, 130, 66


# ---- bh_bases_first_difference -------------------------------------------------------------------------------------------
def _first_difference(worker, a, first_a, b, first_b, count):
    lib, ctx = _lib_ctx(worker)
    idx = ctypes.c_size_t(12345)
    rc = lib.bh_bases_first_difference(ctx, a._h if a is not None else None, first_a, b._h if b is not None else None, first_b,
                                       count, ctypes.byref(idx))
    return rc, idx.value


def _random_records(group, n, tag):
    """records need not be points: the comparison reads bytes"""
    return np.random.default_rng(1000 * group + tag).integers(1, 1 << 63, size=(n, WORDS[group]), dtype=np.uint64)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("group", [1, 2])
def test_first_difference_positions(worker, group, count):
    from bellman_amd.ceremony import bases_first_difference
    from bellman_amd.multiexp import Bases

    base = _random_records(group, count, count)
    a = Bases(worker, group, base)
    cases = [([], count), ([0], 0), ([count - 1], count - 1), ([count - 1, count // 2], count // 2)]
    for places, want in cases:
        for word in (0, WORDS[group] - 1):   # the first 8 bytes of a record, its last 8 bytes only
            other = base.copy()
            for p in set(places):
                other[p, word] ^= np.uint64(1 << 63 if word else 1)
            b = Bases(worker, group, other)
            assert _first_difference(worker, a, 0, b, 0, count) == (0, want), (places, word)
            assert bases_first_difference(worker, b, a) == want
            b.release()
    ident = base.copy()
    ident[count - 1] = 0   # the identity against a point
    b = Bases(worker, group, ident)
    assert _first_difference(worker, a, 0, b, 0, count) == (0, count - 1)
    assert _first_difference(worker, b, 0, a, 0, count) == (0, count - 1)
    assert _first_difference(worker, b, 0, b, 0, count) == (0, count)   # the same handle twice
    assert _first_difference(worker, a, 0, b, 0, count - 1) == (0, count - 1)   # the range ends in front of the difference
    assert _first_difference(worker, a, 0, b, 0, 0) == (0, 0)
    assert _first_difference(worker, a, count, b, count, 0) == (0, 0)
    assert _first_difference(worker, a, 0, b, 1, count)[0] == -2 and _first_difference(worker, a, count + 1, b, 0, 0)[0] == -2
    a.release()
    b.release()


def test_first_difference_offsets_within_one_handle_and_groups(worker):
    from bellman_amd.multiexp import Bases

    for group in (1, 2):
        period = _random_records(group, 70, 7)
        recs = np.concatenate([period, period, period[:60]])   # 200 records of period 70
        recs[140 + 33, 3] ^= np.uint64(2)
        h = Bases(worker, group, recs)
        assert _first_difference(worker, h, 0, h, 70, 70) == (0, 70)
        assert _first_difference(worker, h, 0, h, 70, 130) == (0, 70 + 33)   # record 173 against record 103
        assert _first_difference(worker, h, 70, h, 140, 60) == (0, 33)
        assert _first_difference(worker, h, 1, h, 70, 69) == (0, 0)
        assert _first_difference(worker, h, 130, h, 60, 71)[0] == -2
        h.release()
    g1, g2 = Bases(worker, 1, _random_records(1, 4, 1)), Bases(worker, 2, _random_records(2, 4, 1))
    assert _first_difference(worker, g1, 0, g2, 0, 4)[0] == -2
    assert _first_difference(worker, None, 0, g1, 0, 1)[0] == -2 and _first_difference(worker, g1, 0, None, 0, 1)[0] == -2
    g1.release()
    g2.release()


def test_first_difference_wrapped_handles_past_one_grid(worker):
    """one record more than a single pass of the capped grid covers, in wrapped (live) buffers: the only difference sits in
    the stride's second pass"""
    from bellman_amd.errors import check
    from bellman_amd.multiexp import Bases

    lib, ctx = _lib_ctx(worker)
    shape = (ctypes.c_uint32 * 2)()
    lib.bh_test_compare_shape(shape)
    n = shape[0] * shape[1] + 1
    recs = _random_records(1, n, 99)
    da, db = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bh_dev_alloc(ctx, recs.nbytes, ctypes.byref(da)))
    check(lib.bh_dev_alloc(ctx, recs.nbytes, ctypes.byref(db)))
    try:
        check(lib.bh_dev_upload(ctx, da, recs.ctypes.data_as(ctypes.c_void_p), recs.nbytes))
        check(lib.bh_dev_upload(ctx, db, recs.ctypes.data_as(ctypes.c_void_p), recs.nbytes))
        a, b = Bases.wrap_device(worker, 1, da, n), Bases.wrap_device(worker, 1, db, n)
        assert _first_difference(worker, a, 0, b, 0, n) == (0, n)
        patch = recs[n - 1:].copy()
        patch[0, 11] ^= np.uint64(1 << 40)
        check(lib.bh_dev_upload(ctx, ctypes.c_void_p(db.value + (n - 1) * 96), patch.ctypes.data_as(ctypes.c_void_p), 96))
        assert _first_difference(worker, a, 0, b, 0, n) == (0, n - 1)   # a live view: read as it is when the call runs
        assert _first_difference(worker, a, 0, b, 0, n - 1) == (0, n - 1)
        assert _first_difference(worker, a, 1, b, 1, n - 1) == (0, n - 2)
        check(lib.bh_dev_upload(ctx, ctypes.c_void_p(db.value + 5 * 96), patch.ctypes.data_as(ctypes.c_void_p), 96))
        assert _first_difference(worker, a, 0, b, 0, n) == (0, 5)   # two differences: the smaller index wins
        odd = Bases.wrap_device(worker, 1, ctypes.c_void_p(da.value + 8), 4)
        assert _first_difference(worker, odd, 0, a, 0, 4)[0] == -2   # not 16-byte aligned
        for h in (a, b, odd):
            h.release()
    finally:
        lib.bh_dev_free(ctx, da)
        lib.bh_dev_free(ctx, db)


def test_tau_is_root_of_unity(worker):
    from bellman_amd.ceremony import tau_is_root_of_unity
    from bellman_amd.multiexp import Bases

    m = 8
    omega = pow(7, (Q - 1) // m, Q)   # 7 generates the multiplicative group of Fr
    assert pow(omega, m, Q) == 1 and pow(omega, m // 2, Q) != 1
    for tau, want in ((omega, True), (0x1234567, False)):
        t = Bases(worker, 1, _points(worker, 1, [pow(tau, i, Q) for i in range(2 * m - 1)]))
        assert tau_is_root_of_unity(worker, t, m) is want
        assert tau_is_root_of_unity(worker, t, m // 2) is False
        t.release()


# ---- parameter sets from exponents -----------------------------------------------------------------------------------------
def _exponents(tag, n_h=NH, n_l=NL, n_a=NA, n_ic=0):
    rnd = random.Random("phase2 %s" % (tag,))
    r = lambda n: tuple(rnd.randrange(1, Q) for _ in range(n))  # noqa: E731
    beta, delta = rnd.randrange(1, Q), rnd.randrange(1, Q)
    b = r(n_a)
    return model.Params(alpha_g1=rnd.randrange(1, Q), beta_g1=beta, beta_g2=beta, gamma_g2=rnd.randrange(1, Q) if n_ic else 0,
                        delta_g1=delta, delta_g2=delta, ic=r(n_ic), h=r(n_h), l=r(n_l), a=r(n_a), b_g1=b, b_g2=b)


G1_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "ic", "h", "l", "a", "b_g1")


def _records(worker, p):
    """every element of the set as records: ONE fixed-base launch per group"""
    e1, e2, cuts = [], [], {}
    for name in model.Params._fields:
        v = getattr(p, name)
        v = list(v) if isinstance(v, tuple) else [v]
        dst = e1 if name in G1_FIELDS else e2
        cuts[name] = (len(dst), len(v))
        dst += [0 if x is model.OFF else x for x in v]
    r1, r2 = _points(worker, 1, e1), _points(worker, 2, e2)
    out = {}
    for name, (at, n) in cuts.items():
        out[name] = (r1 if name in G1_FIELDS else r2)[at:at + n].copy()
    if p.delta_g1 is model.OFF:
        out["delta_g1"][0] = cref.g1_from_py(psm.g1_points()["off_curve"][1:])[0]
    if p.delta_g2 is model.OFF:
        out["delta_g2"][0] = cref.g2_from_py(psm.g2_points()["off_curve"])[0]
    return out


def _encode(worker, group, recs):
    from bellman_amd.multiexp import Bases

    lib, ctx = _lib_ctx(worker)
    b = Bases(worker, group, recs)
    out = np.zeros(len(recs) * WORDS[group] * 8, dtype=np.uint8)
    assert lib.bh_bases_write_uncompressed(ctx, b._h, 0, len(recs), out.ctypes.data_as(ctypes.c_void_p)) == 0
    b.release()
    return out.tobytes()


def _device(worker, p, patch=None):
    """the set on the device, made by bh_groth16_params_create; a set with ic also carries gamma_g2 and ic: its
    serialised form gets them spliced in and is read back (unchecked)"""
    from bellman_amd import groth16 as pg

    r = _records(worker, p)
    if patch:
        patch(r)
    made = pg.Parameters(worker, r["alpha_g1"][0], r["beta_g1"][0], r["beta_g2"][0], r["delta_g1"][0], r["delta_g2"][0],
                         r["h"], r["l"], r["a"], r["b_g1"], r["b_g2"])
    if not len(p.ic):
        return made
    raw = made.write()
    made.release()
    at_gamma, at_ic = 96 + 96 + 192, 96 + 96 + 192 + 192 + 96 + 192
    assert raw[at_ic:at_ic + 4] == b"\0\0\0\0"
    raw = (raw[:at_gamma] + _encode(worker, 2, r["gamma_g2"]) + raw[at_gamma + 192:at_ic] + len(p.ic).to_bytes(4, "big") +
           _encode(worker, 1, r["ic"]) + raw[at_ic + 4:])
    return pg.Parameters.read(worker, raw, checked=False)


def _step(worker, before, after, seed, validate_points=False):
    """(return code, failed, bad_vector, bad_index) of bh_groth16_params_verify_step"""
    from bellman_amd.groth16 import ParamsStepReport

    lib, ctx = _lib_ctx(worker)
    rep = ParamsStepReport(0xFFFF, 77, 77)
    rc = lib.bh_groth16_params_verify_step(ctx, before._h, after._h, seed, 1 if validate_points else 0, ctypes.byref(rep))
    return rc, rep.failed, rep.bad_vector, rep.bad_index


def _expect(m):
    return ((0 if m[0] == 0 else INVALID_TRANSCRIPT),) + tuple(m)


# ---- the four sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_h,n_l", [(1, 1), (2, 64), (65, 130), (0, 3)])
def test_sums_equal_the_model(worker, n_h, n_l):
    """unrelated exponents on the two sides: every sum is [sum rho_i x_i]G for its own vector"""
    lib, ctx = _lib_ctx(worker)
    before, after = _exponents(("sums", n_h, n_l, 0), n_h, n_l, 2), _exponents(("sums", n_h, n_l, 1), n_h, n_l, 2)
    db, da = _device(worker, before), _device(worker, after)
    got = {}
    for seed in (SEED_A, SEED_B):
        out = np.zeros((4, 12), dtype=np.uint64)
        rcs = (ctypes.c_int * 4)()
        assert lib.bh_test_phase2_sums(ctx, db._h, da._h, seed, out.ctypes.data_as(ctypes.c_void_p), rcs) == 0
        assert list(rcs) == [0] * 4
        for k, (e, ident) in enumerate(model.sums(before, after, seed)):
            assert not ident
            want = cref.point_mul(1, GEN[1], e) if e else np.zeros(12, np.uint64)
            assert out[k].tobytes() == want.tobytes(), (seed, k)
        got[seed] = out
    assert all(got[SEED_A][k].tobytes() != got[SEED_B][k].tobytes() for k in range(4) if (n_h if k < 2 else n_l))
    assert lib.bh_test_phase2_sums(ctx, db._h, _device(worker, _exponents("sums short", n_h + 1, n_l, 2))._h, SEED_A,
                                   out.ctypes.data_as(ctypes.c_void_p), rcs) == -2


# ---- honest steps ------------------------------------------------------------------------------------------------------------
def _generated(worker, which):
    from bellman_amd import groth16 as pg

    rnd = random.Random("phase2 generated %s" % (which,))
    if which == "mimc25":
        r1cs = pg.R1CS.from_demo(worker, 0, 25, 0, [rnd.randrange(Q) for _ in range(25)])
    else:
        r1cs = pg.R1CS.from_demo(worker, 1, which, 5)
    return pg.Parameters.generate(worker, r1cs, GEN[1], GEN[2], *[rnd.randrange(1, Q) for _ in range(5)])


@pytest.mark.parametrize("which", [1, 2, 9, 130, "mimc25"])
def test_rescale_delta_of_generated_parameters_passes(worker, which):
    params = _generated(worker, which)
    rnd = random.Random(str(which))
    once = params.rescale_delta(rnd.randrange(2, Q))
    twice = once.rescale_delta(rnd.randrange(2, Q))
    for after in (once, twice, params.rescale_delta(1), params):   # one step, two composed, d = 1 (rescaled and as is)
        for flag in (False, True):
            assert _step(worker, params, after, SEED_A, flag) == (0, 0, 0, 0), flag
    assert _step(worker, once, twice, SEED_B, True) == (0, 0, 0, 0)
    assert once.verify_step(twice).failed == 0   # the Python method, a seed from the CSPRNG
    # ... and the step is not symmetric in anything but d -> 1/d: `params` IS `once` rescaled by 1/d
    assert _step(worker, once, params, SEED_A, True) == (0, 0, 0, 0)


# ---- one fault -----------------------------------------------------------------------------------------------------------------
def _faults():
    f = [("h-first", ("exp", "h", 0)), ("h-last", ("exp", "h", NH - 1)), ("l-first", ("exp", "l", 0)), ("l-last", ("exp", "l", NL - 1)),
         ("h-and-l-other-factors", ("rescale_l",)), ("delta-g1-only", ("scalar", "delta_g1")), ("delta-g2-only", ("scalar", "delta_g2")),
         ("deltas-by-different-factors", ("deltas",)), ("h-identity-inside", ("zero", "h", NH // 2))]
    for q in ("a", "b_g1", "b_g2"):
        f += [("%s-first" % q, ("exp", q, 0)), ("%s-last" % q, ("exp", q, NA - 1))]
    f += [("key-%s" % k, ("scalar", k)) for k in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2")] + [("key-ic1", ("exp", "ic", 1))]
    f += [("shape-%s" % q, ("shorter", q)) for q in ("h", "l", "a", "b_g1", "b_g2", "ic")]
    f += [("head-identity-delta-g1", ("set", "delta_g1", 0)), ("head-identity-delta-g2-before", ("set_before", "delta_g2", 0)),
          ("head-off-curve-delta-g1", ("set", "delta_g1", model.OFF)), ("head-off-curve-delta-g2", ("set", "delta_g2", model.OFF))]
    return f


def _apply(before, after, fault):
    kind = fault[0]
    bump = lambda v, i: tuple(x + 1 if k == i else x for k, x in enumerate(v))  # noqa: E731
    if kind == "exp":
        after = after._replace(**{fault[1]: bump(getattr(after, fault[1]), fault[2])})
    elif kind == "zero":
        after = after._replace(**{fault[1]: tuple(0 if k == fault[2] else x for k, x in enumerate(getattr(after, fault[1])))})
    elif kind == "rescale_l":
        after = after._replace(l=model.rescale_delta(before, 0xBAD).l)
    elif kind == "scalar":
        after = after._replace(**{fault[1]: getattr(after, fault[1]) * 3 % Q})
    elif kind == "deltas":
        after = after._replace(delta_g1=after.delta_g1 * 3 % Q, delta_g2=after.delta_g2 * 5 % Q)
    elif kind == "shorter":
        after = after._replace(**{fault[1]: getattr(after, fault[1])[:-1]})
    elif kind == "set":
        after = after._replace(**{fault[1]: fault[2]})
    elif kind == "set_before":
        before = before._replace(**{fault[1]: fault[2]})
    return before, after


@pytest.mark.parametrize("name,fault", _faults(), ids=[f[0] for f in _faults()])
def test_one_fault_gives_the_models_mask_vector_and_index(worker, name, fault):
    with_key = name.startswith("key-") or name == "shape-ic"   # (sets read back from their serialised form: they carry ic)
    before = _exponents("faults", n_ic=3 if with_key else 0)
    before, after = _apply(before, model.rescale_delta(before, 0xD1CE5), fault)
    assert model.step(before, model.rescale_delta(before, 0xD1CE5), SEED_A)[0] in (0, model.HEAD)
    db, da = _device(worker, before), _device(worker, after)
    for seed in (SEED_A, SEED_B):
        want = model.step(before, after, seed)
        assert want[0] != 0
        assert _step(worker, db, da, seed) == _expect(want), seed
    # what the case is about: one fault, one bit - except where delta_g2', which every equation reads, is the fault
    several = {"h-and-l-other-factors": model.L, "delta-g2-only": model.DELTA | model.H | model.L,
               "deltas-by-different-factors": model.DELTA | model.H | model.L}
    one_bit = {"h-": model.H, "l-": model.L, "a-": model.A, "b_g1-": model.B_G1, "b_g2-": model.B_G2, "key-": model.KEY,
               "shape-": model.SHAPE, "head-": model.HEAD, "delta-g1": model.DELTA}
    expected = several[name] if name in several else [v for k, v in one_bit.items() if name.startswith(k)][0]
    assert want[0] == expected, name


def test_several_findings_name_the_first(worker):
    before = _exponents("several", n_ic=2)
    after = model.rescale_delta(before, 77)
    after = after._replace(beta_g2=1, b_g1=(1,) + after.b_g1[1:], b_g2=after.b_g2[:-1] + (1,), h=(1,) + after.h[1:])
    want = model.step(before, after, SEED_A)
    assert want == (model.KEY | model.B_G1 | model.B_G2 | model.H, 0, 2)
    assert _step(worker, _device(worker, before), _device(worker, after), SEED_A) == _expect(want)
    after = after._replace(beta_g2=before.beta_g2)
    want = model.step(before, after, SEED_A)
    assert want == (model.B_G1 | model.B_G2 | model.H, 2, 0)
    assert _step(worker, _device(worker, before), _device(worker, after), SEED_A) == _expect(want)


# ---- BH_STEP_VALIDATE_POINTS ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _outside_subgroup(d_inv):
    """T on the curve and outside the subgroup, and [1/d]T: scaled like every honest point"""
    t = pointgen.g1_on_curve_not_in_subgroup(5)
    return cref.g1_from_py([t, bls.G1.mul(t, d_inv)])


@pytest.mark.parametrize("vector,name,index", [(4, "h", 0), (4, "h", NH - 1), (5, "l", 64)])
def test_validate_points_finds_what_the_equations_cannot(worker, vector, name, index):
    import bellman_amd

    d = 0xD1CE5
    before = _exponents("validate")
    after = model.rescale_delta(before, d)
    pair = _outside_subgroup(pow(d, -1, Q))

    def patch_before(r):
        r[name][index] = pair[0]

    def patch_after(r):
        r[name][index] = pair[1]

    db, da = _device(worker, before, patch_before), _device(worker, after, patch_after)
    # the pairing sees the subgroup component of a point only: consistent scaling passes every equation
    assert _step(worker, db, da, SEED_A) == (0, 0, 0, 0)
    assert _step(worker, db, da, SEED_A, True) == (INVALID_POINT,) + model.step(before, after, SEED_A, bad_points=(vector, index))
    with pytest.raises(bellman_amd.InvalidPoint) as e:
        db.verify_step(da, seed=SEED_A)
    assert (e.value.report.failed, e.value.report.bad_vector, e.value.report.bad_index) == (model.POINTS, vector, index)
    assert db.verify_step(da, seed=SEED_A, validate_points=False).failed == 0


def test_validate_points_identity_and_deltas(worker):
    import bellman_amd

    before = _exponents("validate identity")
    after = model.rescale_delta(before, 9)
    zero = after._replace(l=tuple(0 if i == 129 else x for i, x in enumerate(after.l)))
    db, dz = _device(worker, before), _device(worker, zero)
    want = model.step(before, zero, SEED_A, bad_points=model.validation_finding(zero))
    assert want == (model.POINTS, 5, 129)
    assert _step(worker, db, dz, SEED_A, True) == (POINT_AT_INFINITY,) + want
    assert _step(worker, db, dz, SEED_A) == _expect(model.step(before, zero, SEED_A)) == (INVALID_TRANSCRIPT, model.L, 0, 0)
    with pytest.raises(bellman_amd.InvalidTranscript) as e:
        db.verify_step(dz, seed=SEED_A, validate_points=False)
    assert e.value.report.failed == model.L
    # delta_g1' on the curve and outside the subgroup: HEAD passes it, the validator names vector 6
    def patch(r):
        r["delta_g1"][0] = _outside_subgroup(1)[0]

    assert _step(worker, db, _device(worker, after, patch), SEED_A, True) == (INVALID_POINT, model.POINTS, 6, 0)


# ---- bh_pairing_same_ratio_each ------------------------------------------------------------------------------------------------
def _rows_records(worker, rows):
    cols = list(zip(*rows)) if rows else [(), (), (), ()]
    recs = [_points(worker, 1 if k < 2 else 2, [0 if x is model.OFF else x for x in col]) if rows else
            np.zeros((0, WORDS[1 if k < 2 else 2]), np.uint64) for k, col in enumerate(cols)]
    off1 = cref.g1_from_py(psm.g1_points()["off_curve"][1:])[0]
    off2 = cref.g2_from_py(psm.g2_points()["off_curve"])[0]
    for k, col in enumerate(cols):
        for i, x in enumerate(col):
            if x is model.OFF:
                recs[k][i] = off1 if k < 2 else off2
    return recs


def _mixed_rows(n, tag):
    """equal and unequal ratios interleaved"""
    rnd = random.Random("same ratio %s" % (tag,))
    rows = []
    for i in range(n):
        a, A, d = rnd.randrange(1, Q), rnd.randrange(1, Q), rnd.randrange(1, Q)
        rows.append((a, a * d % Q, A, (A * d + (i % 3 == 1)) % Q))
    return rows


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_same_ratio_each_equals_the_model(worker, n):
    from bellman_amd.ceremony import same_ratio_each

    lib, ctx = _lib_ctx(worker)
    rows = _mixed_rows(n, n)
    want = model.same_ratio(rows)
    assert want == [INVALID_TRANSCRIPT if i % 3 == 1 else 0 for i in range(n)]
    recs = _rows_records(worker, rows)
    assert list(same_ratio_each(worker, *recs)) == want
    verdicts = np.full(n + 1, 99, dtype=np.int32)
    n_bad = ctypes.c_size_t(99)
    assert lib.bh_pairing_same_ratio_each(ctx, *[r.ctypes.data_as(ctypes.c_void_p) for r in recs], n,
                                          verdicts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_bad)) == 0
    assert list(verdicts[:n]) == want and verdicts[n] == 99 and n_bad.value == sum(1 for v in want if v)


def test_same_ratio_each_bad_rows_keep_to_themselves(worker):
    """an identity in each of the four positions, an off-curve point in G1 and in G2 (and beside an identity), between
    good rows whose verdicts must not change"""
    from bellman_amd.ceremony import same_ratio_each

    good = _mixed_rows(9, "neighbours")
    rows = list(good)
    for at, (pos, what) in zip((1, 2, 4, 5, 6, 7, 8), ((0, 0), (1, 0), (2, 0), (3, 0), (1, model.OFF), (2, model.OFF), (3, model.OFF))):
        rows[at] = tuple(what if k == pos else x for k, x in enumerate(rows[at]))
    rows.append((0, model.OFF, 5, 5))   # the identity rule is tested first
    want = model.same_ratio(rows)
    assert want == [0, 7, 7, 0, 7, 7, 6, 6, 6, 7]
    assert list(same_ratio_each(worker, *_rows_records(worker, rows))) == want
    assert list(same_ratio_each(worker, *_rows_records(worker, good))) == model.same_ratio(good)
    assert len(same_ratio_each(worker, *_rows_records(worker, []))) == 0


def test_same_ratio_each_across_the_chunk_edge(worker):
    """BATCH_CHUNK / 2 + 1 rows of three distinct rows repeated: the last row runs in a chunk of its own"""
    from bellman_amd.ceremony import same_ratio_each

    n = 16384 // 2 + 1   # BATCH_CHUNK = 16384 (csrc/fp12.cuh)
    three = [(3, 15, 7, 35), (3, 15, 7, 36), (3, 0, 7, 35)]
    recs3 = _rows_records(worker, three)
    pick = np.arange(n) % 3
    pick[n - 1] = 1   # (n - 1) % 3 = 2 would end on the host-decided row: make the lone row of the last chunk a device one
    rows = [three[k] for k in pick]
    got = same_ratio_each(worker, *[np.ascontiguousarray(r[pick]) for r in recs3])
    assert list(got) == model.same_ratio(rows)


# ---- contributions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
def test_verify_contributions_equals_the_model(worker, n):
    from bellman_amd.ceremony import verify_contributions

    rnd = random.Random("contributions %d" % n)
    delta0 = rnd.randrange(1, Q)
    ds, ss, rs = ([rnd.randrange(2, Q) for _ in range(n)] for _ in range(3))
    good, delta = [], delta0
    for j in range(n):
        good.append(model.contribution(delta, ds[j], ss[j], rs[j]))
        delta = good[-1][0]
    chains = [good]
    for j in range(n):
        d_after, s, d_s, d_r = good[j]
        chains += [good[:j] + [(d_after, s, d_s + 1, d_r)] + good[j + 1:], good[:j] + [(d_after, s, d_s, d_r + 1)] + good[j + 1:],
                   good[:j] + [(d_after + 1, s, d_s, d_r)] + good[j + 1:]]
    # every point of every chain in one launch per group
    e1 = [delta0] + [x for ch in chains for c in ch for x in c[:3]]
    e2 = rs + [c[3] for ch in chains for c in ch]
    r1, r2 = _points(worker, 1, e1), _points(worker, 2, e2)
    for k, ch in enumerate(chains):
        recs = [(r1[1 + 3 * (k * n + j)], r1[2 + 3 * (k * n + j)], r1[3 + 3 * (k * n + j)], r2[n + k * n + j]) for j in range(n)]
        want = model.contributions(delta0, ch, rs)
        assert (k == 0) == (want == [0] * n)
        assert verify_contributions(worker, r1[0], recs, list(r2[:n])) == want, k


def test_contribute_makes_a_step_and_a_proof_that_verify(worker):
    from bellman_amd.ceremony import contribute, verify_contributions

    params = _generated(worker, 9)
    rnd = random.Random("contribute")
    cur, contribs, chal = params, [], _points(worker, 2, [rnd.randrange(1, Q) for _ in range(2)])
    for j in range(2):
        nxt, c = contribute(cur, rnd.randrange(2, Q), _points(worker, 1, [rnd.randrange(1, Q)])[0], chal[j])
        assert _step(worker, cur, nxt, SEED_A, True) == (0, 0, 0, 0)
        assert c[0].tobytes() == nxt.vk()[3].tobytes()
        contribs.append(c)
        cur = nxt
    assert _step(worker, params, cur, SEED_B, True) == (0, 0, 0, 0)
    assert verify_contributions(worker, params.vk()[3], contribs, list(chal)) == [0, 0]
    assert verify_contributions(worker, params.vk()[3], contribs, list(chal[::-1])) == [INVALID_TRANSCRIPT, INVALID_TRANSCRIPT]
    assert verify_contributions(worker, contribs[0][0], contribs[1:], [chal[1]]) == [0]


# ---- concurrency and arguments ---------------------------------------------------------------------------------------------------
def test_four_threads_verify_four_steps(worker):
    sets, wants = [], []
    for k in range(4):
        before = _exponents("thread %d" % k, 65 if k % 2 else 9, 130 if k % 2 else 17, 66 if k % 2 else 5)
        after = model.rescale_delta(before, 1000 + k)
        if k == 2:
            after = after._replace(h=after.h[:3] + (after.h[3] + 1,) + after.h[4:])
        if k == 3:
            after = after._replace(a=after.a[:7] + (after.a[7] + 1,) + after.a[8:])
        sets.append((_device(worker, before), _device(worker, after)))
        wants.append(_expect(model.step(before, after, SEED_A)))
    assert [w[1] for w in wants] == [0, 0, model.H, model.A] and wants[3][2:] == (1, 7)
    alone = [_step(worker, b, a, SEED_A, True) for b, a in sets]
    assert alone == wants
    got = [None] * 4

    def run(k):
        got[k] = [_step(worker, *sets[k], SEED_A, True) for _ in range(3)]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == [[r] * 3 for r in alone]


def test_invalid_arguments(worker):
    lib, ctx = _lib_ctx(worker)
    p = _device(worker, _exponents("args", 2, 2, 2))
    assert lib.bh_groth16_params_verify_step(ctx, None, p._h, SEED_A, 0, None) == -2
    assert lib.bh_groth16_params_verify_step(ctx, p._h, None, SEED_A, 0, None) == -2
    assert lib.bh_groth16_params_verify_step(ctx, p._h, p._h, None, 0, None) == -2
    assert lib.bh_groth16_params_verify_step(None, p._h, p._h, SEED_A, 0, None) == -2
    assert lib.bh_groth16_params_verify_step(ctx, p._h, p._h, SEED_A, 2, None) == -2   # an unknown flag bit
    assert lib.bh_groth16_params_verify_step(ctx, p._h, p._h, SEED_A, 1, None) == 0    # report may be NULL
    one = np.zeros(24, np.uint64)
    v = np.zeros(1, np.int32)
    ptr = one.ctypes.data_as(ctypes.c_void_p)
    assert lib.bh_pairing_same_ratio_each(ctx, None, ptr, ptr, ptr, 1, v.ctypes.data_as(ctypes.c_void_p), None) == -2
    assert lib.bh_pairing_same_ratio_each(ctx, ptr, ptr, ptr, ptr, 1, None, None) == -2
    assert lib.bh_pairing_same_ratio_each(None, ptr, ptr, ptr, ptr, 1, v.ctypes.data_as(ctypes.c_void_p), None) == -2
    assert lib.bh_pairing_same_ratio_each(ctx, None, None, None, None, 0, None, None) == 0
