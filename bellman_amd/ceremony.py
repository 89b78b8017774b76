"""Checking a powers-of-tau transcript before parameters are derived from it (bh_powers_of_tau_verify,
bh_pairing_product_is_one; include/bellman_hip.h).  `Parameters.from_powers_of_tau` validates nothing: this is the check
that the four vectors and beta_g2 are powers of ONE (tau, alpha, beta), by random linear combinations and pairings on the
device.  Not covered: contribution proofs (the contributors' proofs of knowledge), tau being a root of unity of the domain,
and the parsing of any ceremony's file format."""

import ctypes
import secrets

import numpy as np

from . import _lib
from .errors import InvalidData, InvalidTranscript, check

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
