"""The split-scalar point multiplier on the GPU and what is built on it: the ladder kernel against its host build,
bh_point_mul_each_dev, bh_bases_scale_powers, bh_powers_of_tau_contribute and the Python ceremony calls
new_powers_of_tau / contribute_powers_of_tau / verify_powers_of_tau_update.  Inputs are [x_i]G from uploaded exponents
(bh_fixed_base_mul_dev) and the expected records are [x_i s_i mod q]G from the same call, so every comparison is an
equality of records; the exponent model (tests/models/ptau_verify_model.py, tests/models/glv_model.py) predicts every
verdict."""

import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests.models import glv_model as glv  # noqa: E402
from tests.models import ptau_verify_model as model  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401
from tests.test_gpu_ptau_verify import GEN, SEED_A, WORDS, _Device, _lib_ctx, _points  # noqa: E402

Q, LAM = bls.Q, glv.LAMBDA
R = (1 << 256) % Q
SAME_RATIO_FAILS = 10


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _halves(vals):
    return np.frombuffer(b"".join(v.to_bytes(16, "little") for v in vals), dtype=np.uint64).copy()


# ---- the ladder kernel equals its host build ---------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_ladder_kernel_equals_the_host_build(worker, group):
    lib, ctx = _lib_ctx(worker)
    top = (1 << 128) - 1
    pairs = [glv.split(k) for k in glv.corner_scalars()] + [(k1, k2) for _, k1, k2, _ in glv.branch_pairs()]
    pairs += [(top, top), (top, 0), (0, top), (LAM, LAM), (3, 5), (top, 1)]
    pairs = pairs + pairs[::-1]   # the table twice, over other points: neighbours differ in every wavefront
    n = len(pairs)
    assert n > 64   # more than one wavefront
    pts = cref.gen_bases(group, n, a=9, b=14)
    pts[n - 2:] = 0   # identity inputs
    k1, k2 = _halves([a for a, _ in pairs]), _halves([b for _, b in pairs])
    host, dev = np.zeros_like(pts), np.zeros_like(pts)
    assert lib.bh_test_glv_ladder_host(group, _p(pts), _p(k1), _p(k2), n, _p(host)) == 0
    assert lib.bh_test_glv_ladder_dev(ctx, group, _p(pts), _p(k1), _p(k2), n, _p(dev)) == 0
    assert np.array_equal(dev, host)
    assert not dev[n - 2:].any() and not dev[0].any() and dev[1].tobytes() == pts[1].tobytes()   # identity in, k = 0, k = 1


# ---- bh_point_mul_each_dev ---------------------------------------------------------------------------------------------
def _scalar_bytes(scalars, fmt):
    return b"".join(((s % Q) * R % Q if fmt == 1 else s).to_bytes(32, "little") for s in scalars)


@pytest.mark.parametrize("fmt", [0, 1], ids=["canonical", "mont"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("group", [1, 2])
def test_point_mul_each(worker, group, n, fmt):
    """wavefront and block edges; the scalars cycle through the corner list, so every wavefront mixes lengths and bit
    patterns (s = 0 among them); identity records among the inputs; out of place, then in place"""
    from bellman_amd.errors import check

    lib, ctx = _lib_ctx(worker)
    rnd = random.Random(1000 * group + 10 * n + fmt)
    corners = glv.corner_scalars()
    if fmt == 0:
        corners = corners + [Q, Q + 5, (1 << 256) - 1]   # a canonical-format value is taken mod q
    scalars = [corners[(i + n) % len(corners)] for i in range(n)]
    xs = [0 if i % 7 == 3 else rnd.randrange(1, Q) for i in range(n)]
    pts = _points(worker, group, xs)
    want = _points(worker, group, [x * s % Q for x, s in zip(xs, scalars)])
    assert n < 4 or not pts[3].any()
    rec = WORDS[group] * 8
    sc = np.frombuffer(_scalar_bytes(scalars, fmt), dtype=np.uint64).copy()
    d_in, d_sc, d_out = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    for d, size in ((d_in, n * rec), (d_sc, n * 32), (d_out, n * rec)):
        check(lib.bh_dev_alloc(ctx, size, ctypes.byref(d)))
    try:
        check(lib.bh_dev_upload(ctx, d_in, _p(pts), n * rec))
        check(lib.bh_dev_upload(ctx, d_sc, _p(sc), n * 32))
        out, inplace, kept = np.zeros_like(pts), np.zeros_like(pts), np.zeros_like(pts)
        check(lib.bh_point_mul_each_dev(ctx, group, d_in, d_sc, n, fmt, d_out, None))
        check(lib.bh_dev_download(ctx, _p(out), d_out, n * rec))
        check(lib.bh_dev_download(ctx, _p(kept), d_in, n * rec))
        check(lib.bh_point_mul_each_dev(ctx, group, d_in, d_sc, n, fmt, d_in, None))
        check(lib.bh_dev_download(ctx, _p(inplace), d_in, n * rec))
    finally:
        for d in (d_in, d_sc, d_out):
            lib.bh_dev_free(ctx, d)
    assert np.array_equal(out, want)
    assert np.array_equal(kept, pts)        # out of place leaves the input alone
    assert np.array_equal(inplace, want)


def test_point_mul_each_arguments(worker):
    lib, ctx = _lib_ctx(worker)
    assert lib.bh_point_mul_each_dev(ctx, 1, None, None, 0, 0, None, None) == 0   # n = 0 does nothing
    assert lib.bh_point_mul_each_dev(ctx, 3, None, None, 0, 0, None, None) == -2
    assert lib.bh_point_mul_each_dev(ctx, 1, None, None, 0, 2, None, None) == -2
    assert lib.bh_point_mul_each_dev(ctx, 2, None, None, 4, 1, None, None) == -2


def test_python_point_mul_each(worker):
    from bellman_amd import point_mul_each

    rnd = random.Random(77)
    xs, ss = [rnd.randrange(1, Q) for _ in range(5)], [rnd.randrange(Q) for _ in range(5)]
    sc = np.frombuffer(_scalar_bytes(ss, 0), dtype=np.uint64).reshape(5, 4)
    for group in (1, 2):
        got = point_mul_each(worker, group, _points(worker, group, xs), sc)
        assert np.array_equal(got, _points(worker, group, [x * s % Q for x, s in zip(xs, ss)]))


# ---- bh_bases_scale_powers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 130])
@pytest.mark.parametrize("group", [1, 2])
def test_scale_powers_equals_the_exponent_model(worker, group, n):
    from bellman_amd.multiexp import Bases

    rnd = random.Random(31 * n + group)
    xs = [rnd.randrange(1, Q) for _ in range(n)]
    before = Bases(worker, group, _points(worker, group, xs))
    for c in (1, rnd.randrange(2, Q)):
        for g in (1, Q - 1, 7, rnd.randrange(2, Q)):
            after = before.scale_powers(c, g)
            assert len(after) == n and after.group == group
            want = _points(worker, group, [x * c * pow(g, i, Q) % Q for i, x in enumerate(xs)])
            assert np.array_equal(after.download(), want), (c, g)
            after.release()
    assert np.array_equal(before.download(), _points(worker, group, xs))   # the input handle is left unchanged


def test_scale_powers_refuses_zero(worker):
    from bellman_amd import UnexpectedIdentity
    from bellman_amd.multiexp import Bases

    b = Bases(worker, 1, _points(worker, 1, [1, 2, 3]))
    for c, g in ((0, 5), (5, 0), (Q, 5), (5, Q)):
        with pytest.raises(UnexpectedIdentity):
            b.scale_powers(c, g)


# ---- bh_powers_of_tau_contribute -----------------------------------------------------------------------------------------
def _secrets(tag):
    rnd = random.Random("ptau contribute %s" % (tag,))
    return rnd.randrange(2, Q), rnd.randrange(2, Q), rnd.randrange(2, Q)


def _transcript(dev):
    from bellman_amd.ceremony import PowersOfTau

    return PowersOfTau(*dev.args())


def _proof_inputs(tag):
    """({x: exponent of s_x}, {x: exponent of r_x}) for the three secrets"""
    rnd = random.Random("ptau proofs %s" % (tag,))
    return {x: rnd.randrange(1, Q) for x in ("tau", "alpha", "beta")}, {x: rnd.randrange(1, Q) for x in ("tau", "alpha", "beta")}


def _proof_points(worker, sigma, rho):
    s = {x: _points(worker, 1, [e])[0] for x, e in sigma.items()}
    r = {x: _points(worker, 2, [e])[0] for x, e in rho.items()}
    return s, r


def _contribute(worker, tr_dev, secrets, tag="p"):
    from bellman_amd.ceremony import contribute_powers_of_tau

    sigma, rho = _proof_inputs(tag)
    s, r = _proof_points(worker, sigma, rho)
    after, proofs = contribute_powers_of_tau(worker, tr_dev, *secrets, s, r)
    return after, proofs, r


def _assert_is(worker, transcript, tr_model):
    for v in range(4):
        group = 2 if v == 1 else 1
        assert np.array_equal(transcript[v].download(), _points(worker, group, tr_model.vec[v])), v
    assert np.array_equal(transcript.beta_g2, _points(worker, 2, [tr_model.beta2])[0])


@pytest.mark.parametrize("n1,n", [(2, 2), (9, 9), (130, 65)])
def test_contribution_equals_the_exponent_model(worker, n1, n):
    from bellman_amd.ceremony import verify_powers_of_tau

    tau, alpha, beta = _secrets(("before", n1, n))
    t, a, b = _secrets(("step", n1, n))
    before = _transcript(_Device(worker, model.Transcript.consistent(tau, alpha, beta, n1, n)))
    after, proofs, _ = _contribute(worker, before, (t, a, b))
    want = model.Transcript.consistent(tau * t % Q, alpha * a % Q, beta * b % Q, n1, n)
    _assert_is(worker, after, want)
    assert model.mask(want, SEED_A) == 0
    assert verify_powers_of_tau(worker, *after, seed=SEED_A, validate_points=False).failed == 0
    assert verify_powers_of_tau(worker, *after, seed=SEED_A, validate_points=True).failed == 0
    # a second contribution: the same records as ONE contribution with the product secrets
    t2, a2, b2 = _secrets(("step 2", n1, n))
    twice, _, _ = _contribute(worker, after, (t2, a2, b2))
    once, _, _ = _contribute(worker, before, (t * t2 % Q, a * a2 % Q, b * b2 % Q))
    for v in range(4):
        assert np.array_equal(twice[v].download(), once[v].download())
    assert np.array_equal(twice.beta_g2, once.beta_g2)
    # the proofs: (s, [x]s, [x]r)
    sigma, rho = _proof_inputs("p")
    for x, secret in zip(("tau", "alpha", "beta"), (t, a, b)):
        s, xs, xr = proofs[x]
        assert np.array_equal(s, _points(worker, 1, [sigma[x]])[0])
        assert np.array_equal(xs, _points(worker, 1, [sigma[x] * secret])[0])
        assert np.array_equal(xr, _points(worker, 2, [rho[x] * secret])[0])


def test_contribution_refuses_zero_secrets_and_wrong_groups(worker):
    from bellman_amd import UnexpectedIdentity
    from bellman_amd.ceremony import _PowersOfTau
    from bellman_amd.multiexp import _fr_mont

    lib, ctx = _lib_ctx(worker)
    dev = _Device(worker, model.Transcript.consistent(*_secrets("args"), 3, 2))
    before = _transcript(dev)
    for secrets in ((0, 2, 3), (2, 0, 3), (2, 3, Q)):
        with pytest.raises(UnexpectedIdentity):
            _contribute(worker, before, secrets)
    out, beta_g2 = (ctypes.c_void_p * 4)(), np.zeros(24, dtype=np.uint64)
    sc = [_fr_mont(5), _fr_mont(6), _fr_mont(7)]
    h = [x._h for x in dev.bases]
    for handles in ((h[1], h[1], h[2], h[3]), (h[0], h[0], h[2], h[3]), (h[0], h[1], h[1], h[3]), (h[0], h[1], h[2], None)):
        t = _PowersOfTau(*handles, dev.beta_g2.ctypes.data)
        assert lib.bh_powers_of_tau_contribute(ctx, ctypes.byref(t), *sc, out, _p(beta_g2)) == -2
        assert not any(out)
    assert lib.bh_powers_of_tau_contribute(ctx, None, *sc, out, _p(beta_g2)) == -2


# ---- new_powers_of_tau -----------------------------------------------------------------------------------------------------
def test_starting_transcript_verifies_and_is_the_fixed_point_of_unit_secrets(worker):
    from bellman_amd.ceremony import new_powers_of_tau, verify_powers_of_tau

    start = new_powers_of_tau(worker, 9, 5)
    assert [len(v) for v in start[:4]] == [9, 5, 5, 5]
    _assert_is(worker, start, model.Transcript.consistent(1, 1, 1, 9, 5))
    assert np.array_equal(start.beta_g2, GEN[2])
    assert verify_powers_of_tau(worker, *start, seed=SEED_A).failed == 0
    same, _, _ = _contribute(worker, start, (1, 1, 1))
    _assert_is(worker, same, model.Transcript.consistent(1, 1, 1, 9, 5))


# ---- verify_powers_of_tau_update ---------------------------------------------------------------------------------------------
N1, N = 9, 9


def _rows(before, after, secrets_proved, rho_used, rho_checked):
    """the six verdicts in the exponent: row (a, b, A, B) holds iff a B = b A mod q"""
    sigma, _ = _proof_inputs("p")
    step = ((0, 1), (2, 0), (3, 0))
    out = []
    for i, x in enumerate(("tau", "alpha", "beta")):
        A, B = rho_checked[x], rho_used[x] * secrets_proved[x] % Q
        v, at = step[i]
        for a, b in ((sigma[x], sigma[x] * secrets_proved[x] % Q), (before.vec[v][at], after.vec[v][at])):
            out.append(0 if (a * B - b * A) % Q == 0 else SAME_RATIO_FAILS)
    return out


def _update_case(worker, fault):
    """(report, expected mask, expected rows, expected generators_unchanged) for one fault (None: an honest update)"""
    from bellman_amd.ceremony import PowersOfTau, verify_powers_of_tau_update
    from bellman_amd.multiexp import Bases

    tau, alpha, beta = _secrets("update before")
    t, a, b = _secrets("update step")
    tr_before = model.Transcript.consistent(tau, alpha, beta, N1, N)
    before = _transcript(_Device(worker, tr_before))
    applied = (t, (a + 1) % Q if fault == "alpha-differs" else a, b)
    after, proofs, r = _contribute(worker, before, applied)
    tr_after = model.Transcript.consistent(tau * applied[0] % Q, alpha * applied[1] % Q, beta * applied[2] % Q, N1, N)
    proved = {"tau": t, "alpha": a, "beta": b}
    _, rho = _proof_inputs("p")
    rho_used = dict(rho)
    if fault == "alpha-differs":   # the proof is an honest proof of a, the vector was scaled by a + 1
        proofs["alpha"] = (proofs["alpha"][0], _points(worker, 1, [_proof_inputs("p")[0]["alpha"] * a])[0],
                           _points(worker, 2, [rho["alpha"] * a])[0])
    if fault == "foreign-challenge":   # tau's proof was made against another challenge point
        rho_used["tau"] = (rho["tau"] + 1) % Q
        proofs["tau"] = (proofs["tau"][0], proofs["tau"][1], _points(worker, 2, [rho_used["tau"] * t])[0])
    if fault in ("point-replaced", "generator-changed"):
        at = 5 if fault == "point-replaced" else 0
        tr_after.vec[0][at] = (tr_after.vec[0][at] + 1) % Q
        recs = after[0].download()
        recs[at] = _points(worker, 1, [tr_after.vec[0][at]])[0]
        after = PowersOfTau(Bases(worker, 1, recs), *after[1:])
    if fault == "beta-g2-unscaled":
        tr_after.beta2 = tr_before.beta2
        after = PowersOfTau(*after[:4], before.beta_g2)
    report = verify_powers_of_tau_update(worker, before, after, proofs, r, seed=SEED_A)
    return report, model.mask(tr_after, SEED_A), _rows(tr_before, tr_after, proved, rho_used, rho), fault != "generator-changed"


def test_honest_update_passes(worker):
    report, mask, rows, same = _update_case(worker, None)
    assert (mask, rows, same) == (0, [0] * 6, True)
    assert (report.transcript_failed, report.rows, report.generators_unchanged, report.ok) == (0, [0] * 6, True, True)


@pytest.mark.parametrize("fault,mask,rows", [
    ("point-replaced", model.TAU_G1, [0, 0, 0, 0, 0, 0]),
    ("alpha-differs", 0, [0, 0, 0, 10, 0, 0]),
    ("foreign-challenge", 0, [10, 10, 0, 0, 0, 0]),
    ("generator-changed", None, [0, 0, 0, 0, 0, 0]),
    ("beta-g2-unscaled", model.BETA_G2, [0, 0, 0, 0, 0, 0]),
])
def test_one_fault_gives_the_models_verdict_and_changes_no_other(worker, fault, mask, rows):
    report, want_mask, want_rows, same = _update_case(worker, fault)
    assert want_rows == rows and (mask is None or want_mask == mask)   # what the exponent model predicts
    if fault == "generator-changed":   # every equation that reads g1 = T'[0]
        assert want_mask == model.TAU_G1_G2 | model.TAU_G1 | model.TAU_G2 | model.BETA_G2
    assert report.transcript_failed == want_mask
    assert report.rows == want_rows
    assert report.generators_unchanged == same
    assert not report.ok
