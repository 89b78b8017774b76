"""Checking a powers-of-tau transcript before parameters are derived from it (bh_powers_of_tau_verify,
bh_pairing_product_is_one; include/bellman_hip.h).  `Parameters.from_powers_of_tau` validates nothing: this is the check
that the four vectors and beta_g2 are powers of ONE (tau, alpha, beta), by random linear combinations and pairings on the
device.  For the circuit-specific ceremony that follows (contributors rescaling delta): `Parameters.verify_step` checks one
step, `contribute` / `verify_contributions` make and check the contribution proofs (bh_pairing_same_ratio_each),
`tau_is_root_of_unity` is the test a transcript needs beside its consistency.  Not covered: deriving the challenge points
(hashing a ceremony's transcript to G2) and the parsing of any ceremony's file format."""

import ctypes
import secrets

import numpy as np

from . import _lib
from .errors import InvalidData, InvalidTranscript, check

_Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
VALIDATE_POINTS = 1
FAILED_HEAD, FAILED_TAU_G1_G2, FAILED_TAU_G1, FAILED_TAU_G2 = 0x01, 0x02, 0x04, 0x08
FAILED_ALPHA, FAILED_BETA, FAILED_BETA_G2, FAILED_POINTS = 0x10, 0x20, 0x40, 0x80


class PtauReport(ctypes.Structure):
    """bh_ptau_report: `failed` = the FAILED_* bits; with FAILED_POINTS `bad_vector` (0 tau_g1, 1 tau_g2, 2 alpha_tau_g1,
    3 beta_tau_g1) and `bad_index` name the first bad point"""
    _fields_ = [("failed", ctypes.c_uint32), ("bad_vector", ctypes.c_uint32), ("bad_index", ctypes.c_size_t)]


class _PowersOfTau(ctypes.Structure):
    _fields_ = [("tau_g1", ctypes.c_void_p), ("tau_g2", ctypes.c_void_p), ("alpha_tau_g1", ctypes.c_void_p),
                ("beta_tau_g1", ctypes.c_void_p), ("beta_g2", ctypes.c_void_p)]


def verify_powers_of_tau(worker, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, seed=None, validate_points=True):
    """Raises InvalidTranscript (with `.report`) unless tau_g1 (>= 2 points), tau_g2 (>= 2), alpha_tau_g1, beta_tau_g1 (>= 1;
    all `Bases`, checked over their whole length) and beta_g2 (one affine G2 record, [24] uint64) are consistent powers of
    one (tau, alpha, beta).  validate_points=True first puts every point through `Bases.validate(checked=True,
    forbid_identity=True)`: InvalidPoint / PointAtInfinity with `.report` naming the vector and the index.  `seed`: 32
    bytes from which the coefficients of the linear combinations are expanded on the device; it MUST be chosen after the
    transcript is fixed and come from a CSPRNG - left None it is drawn from secrets.token_bytes.  Returns the report
    (failed == 0)."""
    seed = secrets.token_bytes(32) if seed is None else bytes(seed)
    assert len(seed) == 32
    b2 = np.ascontiguousarray(beta_g2, dtype=np.uint64).reshape(24)
    t = _PowersOfTau(*[x._h if x is not None else None for x in (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1)], b2.ctypes.data)
    rep = PtauReport()
    rc = _lib.load().bh_powers_of_tau_verify(worker.ctx, ctypes.byref(t), seed, VALIDATE_POINTS if validate_points else 0,
                                             ctypes.byref(rep))
    if rc == 10:
        raise InvalidTranscript(rep)
    try:
        check(rc, "verify_powers_of_tau")
    except InvalidData as e:
        e.report = rep
        raise
    return rep


def pairing_product_is_one(worker, g1_points, g2_points):
    """prod_i e(P_i, Q_i) == 1 over affine records ([n, 12] and [n, 24] uint64) on the device; a pair with the identity on
    either side contributes 1, no pairs give True.  Raises InvalidPoint for a point off its curve; subgroup membership is
    the caller's business, as for verify_proof."""
    p = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 12)
    q = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 24)
    assert len(p) == len(q)
    one = ctypes.c_int(0)
    check(_lib.load().bh_pairing_product_is_one(worker.ctx, p.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p),
                                                len(p), ctypes.byref(one)), "pairing_product_is_one")
    return bool(one.value)


# ---- a circuit-specific ceremony: one contributor's step and the proofs that go with it ---------------------------------------
# `Parameters.verify_step` (groth16.py) checks that a step changed delta alone.  What follows is the rest of a receiver's
# work, on top of bh_bases_first_difference, bh_pairing_same_ratio_each and the host's bh_point_mul.  THE CHALLENGE POINT
# r_j OF A CONTRIBUTION IS THE CALLER'S: a ceremony derives it by hashing its transcript so far to G2, and that hash belongs
# with the ceremony's file format, which this library does not parse.
def bases_first_difference(worker, a, b, first_a=0, first_b=0, count=None):
    """The first i < count at which record first_a + i of `a` differs from record first_b + i of `b` (two `Bases` of one
    group, or one handle twice), `count` when the ranges hold the same records (bh_bases_first_difference).  Records are
    compared as stored; count=None: as many as both handles hold behind their offsets."""
    if count is None:
        count = min(len(a) - first_a, len(b) - first_b)
    idx = ctypes.c_size_t(0)
    check(_lib.load().bh_bases_first_difference(worker.ctx, a._h, first_a, b._h, first_b, count, ctypes.byref(idx)),
          "bases_first_difference")
    return idx.value


def same_ratio_each(worker, a_g1, b_g1, A_g2, B_g2):
    """One verdict per row over affine records ([n, 12] / [n, 24] uint64): 0 iff e(a_i, B_i) == e(b_i, A_i), that is
    b_i / a_i = B_i / A_i; 7 (point at infinity) when one of the row's four points is the identity - a ratio through the
    identity proves nothing -, 6 when one is off its curve, 10 when the equation fails (bh_pairing_same_ratio_each).  A bad
    row changes no other row's verdict.  Subgroup membership is the caller's business.  Returns an int32 array."""
    arrs = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, w) for x, w in ((a_g1, 12), (b_g1, 12), (A_g2, 24), (B_g2, 24))]
    n = len(arrs[0])
    assert all(len(x) == n for x in arrs)
    verdicts = np.zeros(n, dtype=np.int32)
    check(_lib.load().bh_pairing_same_ratio_each(worker.ctx, *[x.ctypes.data_as(ctypes.c_void_p) for x in arrs], n,
                                                 verdicts.ctypes.data_as(ctypes.c_void_p), None), "same_ratio_each")
    return verdicts


def _mul(group, point, k):
    out = np.zeros(12 if group == 1 else 24, dtype=np.uint64)
    pt = np.ascontiguousarray(point, dtype=np.uint64)
    sc = np.frombuffer((k % _Q).to_bytes(32, "little"), dtype=np.uint64)
    _lib.load().bh_point_mul(group, out.ctypes.data_as(ctypes.c_void_p), pt.ctypes.data_as(ctypes.c_void_p),
                             sc.ctypes.data_as(ctypes.c_void_p))
    return out


def contribute(params, d, s, challenge_g2):
    """One contributor's step: (params.rescale_delta(d), contribution) with contribution = (delta_g1_after, s, [d]s,
    [d]challenge) - `s` an affine G1 record of the contributor's choice (not the identity), `challenge_g2` the affine G2
    challenge point r of this contribution, which the CALLER derives (by hashing the ceremony's transcript to G2).  The
    pair (s, [d]s) against (r, [d]r) shows knowledge of d, and the same G2 pair ties d to the step delta_g1 -> [d]delta_g1."""
    after = params.rescale_delta(d)
    return after, (after.vk()[3], np.ascontiguousarray(s, dtype=np.uint64), _mul(1, s, d), _mul(2, challenge_g2, d))


def verify_contributions(worker, delta_g1_first, contributions, challenges):
    """One verdict per contribution of a chain: `contributions[j]` as `contribute` returns it, `challenges[j]` the affine G2
    challenge point r_j (the caller's, see `contribute`), `delta_g1_first` the delta_g1 the first contribution started
    from.  Two rows per contribution go through ONE same_ratio_each call: (s, [d]s) against (r, [d]r), and (delta_prev,
    delta_after) against the same G2 pair, delta_prev being the previous contribution's delta_after.  The verdict is the
    first nonzero code of the two rows (0: the contribution holds).  That the parameters' delta_g1 IS the last
    delta_after, and that each step changed delta alone, is `Parameters.verify_step`'s part."""
    n = len(contributions)
    a, b, A, B = (np.zeros((2 * n, 12), np.uint64), np.zeros((2 * n, 12), np.uint64), np.zeros((2 * n, 24), np.uint64),
                  np.zeros((2 * n, 24), np.uint64))
    prev = np.ascontiguousarray(delta_g1_first, dtype=np.uint64)
    for j, ((delta_after, s, ds, dr), r) in enumerate(zip(contributions, challenges)):
        a[2 * j], b[2 * j], a[2 * j + 1], b[2 * j + 1] = s, ds, prev, delta_after
        A[2 * j] = A[2 * j + 1] = r
        B[2 * j] = B[2 * j + 1] = dr
        prev = np.ascontiguousarray(delta_after, dtype=np.uint64)
    rows = same_ratio_each(worker, a, b, A, B)
    return [int(rows[2 * j]) or int(rows[2 * j + 1]) for j in range(n)]


def tau_is_root_of_unity(worker, tau_g1, m):
    """Is tau an m-th root of unity - is [tau^m]G1 = tau_g1[m] equal to G1 = tau_g1[0]?  Such a transcript passes
    verify_powers_of_tau and gives unusable parameters (t(tau) = 0) for the domain of size m.  `tau_g1`: a `Bases` of more
    than m points.  One record compared on the device."""
    return bases_first_difference(worker, tau_g1, tau_g1, 0, m, 1) == 1
