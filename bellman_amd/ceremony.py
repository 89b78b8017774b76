"""Checking a powers-of-tau transcript before parameters are derived from it (bh_powers_of_tau_verify,
bh_pairing_product_is_one; include/bellman_hip.h).  `Parameters.from_powers_of_tau` validates nothing: this is the check
that the four vectors and beta_g2 are powers of ONE (tau, alpha, beta), by random linear combinations and pairings on the
device.  For the circuit-specific ceremony that follows (contributors rescaling delta): `Parameters.verify_step` checks one
step, `contribute` / `verify_contributions` make and check the contribution proofs (bh_pairing_same_ratio_each),
`tau_is_root_of_unity` is the test a transcript needs beside its consistency.  Producing a transcript:
`new_powers_of_tau`, `contribute_powers_of_tau` (bh_powers_of_tau_contribute) and the receiver's
`verify_powers_of_tau_update`.  Not covered: deriving the challenge points
(hashing a ceremony's transcript to G2) and the parsing of any ceremony's file format."""

import ctypes
import secrets

import numpy as np

from . import _abi, _lib
from ._abi import C
from .errors import InvalidData, InvalidTranscript, check

_Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
VALIDATE_POINTS = C.BH_PTAU_VALIDATE_POINTS
FAILED_HEAD, FAILED_TAU_G1_G2, FAILED_TAU_G1, FAILED_TAU_G2, FAILED_ALPHA, FAILED_BETA, FAILED_BETA_G2, FAILED_POINTS = (
    getattr(C, "BH_PTAU_FAILED_" + x) for x in ("HEAD", "TAU_G1_G2", "TAU_G1", "TAU_G2", "ALPHA", "BETA", "BETA_G2", "POINTS"))
# bh_ptau_report: `failed` = the FAILED_* bits; with FAILED_POINTS `bad_vector` (0 tau_g1, 1 tau_g2, 2 alpha_tau_g1,
# 3 beta_tau_g1) and `bad_index` name the first bad point
PtauReport = _abi.STRUCTS["bh_ptau_report"]
_PowersOfTau = _abi.STRUCTS["bh_powers_of_tau"]


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
    if rc == C.BH_ERR_INVALID_TRANSCRIPT:
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


# ---- a powers-of-tau ceremony: the starting transcript, one contributor's update, the receiver's check of it -------------------
# bh_powers_of_tau_contribute multiplies every point of the four vectors by its power of the contributor's secrets (the
# split-scalar multiplier of csrc/glv.cuh); the check is assembled from the calls above.  AS FOR `contribute`, THE CHALLENGE
# POINTS ARE THE CALLER'S, and so are the file formats.
_P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
_G1_GENERATOR = (   # the generators of the Zcash BLS12-381 specification, canonical coordinates
    0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
    0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
_G2_GENERATOR = (
    0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
    0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E,
    0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
    0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)
SECRETS = ("tau", "alpha", "beta")


def _record(coords):
    """canonical Fp coordinates -> one affine Montgomery record (uint64 words)"""
    return np.frombuffer(b"".join((c * (1 << 384) % _P).to_bytes(48, "little") for c in coords), dtype=np.uint64).copy()


class PowersOfTau(tuple):
    """(tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2): four `Bases` and one affine G2 record - the argument order of
    verify_powers_of_tau and Parameters.from_powers_of_tau, so `*transcript` passes it on"""
    __slots__ = ()

    def __new__(cls, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2):
        return tuple.__new__(cls, (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, np.ascontiguousarray(beta_g2, dtype=np.uint64).reshape(24)))

    tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2 = (property(lambda self, i=i: self[i]) for i in range(5))


def new_powers_of_tau(worker, n_g1, n):
    """The transcript a ceremony starts from, tau = alpha = beta = 1: every element the generator of its group (n_g1 points
    of tau_g1, n of each other vector)."""
    from .multiexp import Bases

    g1, g2 = _record(_G1_GENERATOR), _record(_G2_GENERATOR)
    return PowersOfTau(Bases(worker, 1, np.tile(g1, (n_g1, 1))), Bases(worker, 2, np.tile(g2, (n, 1))),
                       Bases(worker, 1, np.tile(g1, (n, 1))), Bases(worker, 1, np.tile(g1, (n, 1))), g2)


def contribute_powers_of_tau(worker, transcript, tau, alpha, beta, s_g1, challenges_g2):
    """One contributor's update of a transcript (bh_powers_of_tau_contribute): (new_transcript, proofs) with T'[i] =
    [tau^i]T[i], U'[i] = [tau^i]U[i], A'[i] = [alpha tau^i]A[i], B'[i] = [beta tau^i]B[i], beta_g2' = [beta]beta_g2 over the
    whole length of every vector, and proofs[x] = (s_x, [x]s_x, [x]r_x) for x in "tau", "alpha", "beta" - the convention
    of `contribute`: s_g1[x] an affine G1 record of the contributor's choice (not the identity), challenges_g2[x] the
    affine G2 challenge point r_x, which the CALLER derives (by hashing the ceremony's transcript to G2).  tau, alpha,
    beta: integers mod q, the contributor's secrets; zero raises UnexpectedIdentity.  Validates nothing: run
    verify_powers_of_tau(validate_points=True) over a transcript before contributing to it."""
    from .multiexp import Bases, _fr_mont

    secret = dict(zip(SECRETS, (tau, alpha, beta)))
    t = _PowersOfTau(*[b._h for b in transcript[:4]], transcript.beta_g2.ctypes.data)
    out = (ctypes.c_void_p * 4)()
    beta_g2 = np.zeros(24, dtype=np.uint64)
    check(_lib.load().bh_powers_of_tau_contribute(worker.ctx, ctypes.byref(t), *[_fr_mont(secret[x]) for x in SECRETS], out,
                                                  beta_g2.ctypes.data_as(ctypes.c_void_p)), "contribute_powers_of_tau")
    vecs = []
    for v, before in enumerate(transcript[:4]):
        b = Bases.__new__(Bases)
        b.worker, b.group, b.n, b._h = worker, before.group, len(before), ctypes.c_void_p(out[v])
        vecs.append(b)
    proofs = {x: (np.ascontiguousarray(s_g1[x], dtype=np.uint64), _mul(1, s_g1[x], secret[x]), _mul(2, challenges_g2[x], secret[x]))
              for x in SECRETS}
    return PowersOfTau(*vecs, beta_g2), proofs


class PtauUpdateReport:
    """What verify_powers_of_tau_update found: `transcript_failed` = the FAILED_* bits of verify_powers_of_tau(after),
    `rows` = the six same-ratio verdicts (2 i: the proof of SECRETS[i] itself, 2 i + 1: that secret against the step
    T[1] / A[0] / B[0]), `generators_unchanged` = T[0] and U[0] are the records of `before`; `ok` when all of it holds"""

    def __init__(self, transcript_failed, rows, generators_unchanged):
        self.transcript_failed, self.rows, self.generators_unchanged = transcript_failed, rows, generators_unchanged
        self.ok = transcript_failed == 0 and not any(rows) and generators_unchanged


def verify_powers_of_tau_update(worker, before, after, proofs, challenges_g2, seed=None, validate_points=True):
    """The receiver's check that `after` is `before` updated by ONE contributor who knows the secrets behind `proofs`
    (as contribute_powers_of_tau returns them; challenges_g2[x] the challenge point the receiver derived).  Three steps,
    existing calls only:
      1. verify_powers_of_tau(after): `after` is powers of one (tau', alpha', beta') over g1' = T'[0], g2' = U'[0];
      2. one same_ratio_each call of six rows - for each secret x: (s_x, [x]s_x) against (r_x, [x]r_x), knowledge of x;
         and (T[1], T'[1]) / (A[0], A'[0]) / (B[0], B'[0]) against the same G2 pair, the step taken IS x;
      3. bases_first_difference: T'[0] = T[0] and U'[0] = U[0], the generators are unchanged.
    That is the whole update: a consistent `after` is determined by its generators and its three secrets; 3 fixes the
    generators, and the step rows give tau' = tau x_tau from T[1], alpha' = alpha x_alpha from A[0] = [alpha]g1, beta' =
    beta x_beta from B[0] - every other element, beta_g2 included (equation BETA_G2 of step 1), then follows.  `before`
    is assumed verified (it was the previous `after`).  With the caller: deriving the challenge points from the
    ceremony's transcript, and the file formats.  `seed`: the rule of verify_powers_of_tau.  Points that fail
    validation raise as there.  Returns a PtauUpdateReport; nothing is raised for a failed check."""
    try:
        failed = verify_powers_of_tau(worker, *after, seed=seed, validate_points=validate_points).failed
    except InvalidTranscript as e:
        failed = e.report.failed
    a, b, A, B = np.zeros((6, 12), np.uint64), np.zeros((6, 12), np.uint64), np.zeros((6, 24), np.uint64), np.zeros((6, 24), np.uint64)
    step = ((0, 1), (2, 0), (3, 0))   # (vector, index) of the element a secret's step is read from
    for i, x in enumerate(SECRETS):
        s, xs, xr = proofs[x]
        v, at = step[i]
        a[2 * i], b[2 * i] = s, xs
        a[2 * i + 1], b[2 * i + 1] = before[v].download(at, 1)[0], after[v].download(at, 1)[0]
        A[2 * i] = A[2 * i + 1] = challenges_g2[x]
        B[2 * i] = B[2 * i + 1] = xr
    rows = [int(r) for r in same_ratio_each(worker, a, b, A, B)]
    same = all(bases_first_difference(worker, before[v], after[v], 0, 0, 1) == 1 for v in (0, 1))
    return PtauUpdateReport(failed, rows, same)


def tau_is_root_of_unity(worker, tau_g1, m):
    """Is tau an m-th root of unity - is [tau^m]G1 = tau_g1[m] equal to G1 = tau_g1[0]?  Such a transcript passes
    verify_powers_of_tau and gives unusable parameters (t(tau) = 0) for the domain of size m.  `tau_g1`: a `Bases` of more
    than m points.  One record compared on the device."""
    return bases_first_difference(worker, tau_g1, tau_g1, 0, m, 1) == 1
