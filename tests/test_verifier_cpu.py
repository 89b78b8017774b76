"""The pairing arithmetic of the verifier (bellman_amd/csrc/fp12.cuh) on the host: its Frobenius constants recomputed from
p, full pairings compiled for the host against oracle/pyref, and the Python error mapping.  No device compute here."""

import ctypes
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bellman_amd import _lib  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from oracle.pyref import pairing as pyp  # noqa: E402

P, Q = bls.P, bls.Q
R = 1 << 384
HEADER = os.path.join(ROOT, "bellman_amd", "csrc", "fp12.cuh")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libbellman_hip_test.so not built")
    return _lib.load()


def _table(name, text):
    """the hex words of the constexpr table `m` inside FrobConsts::<name>, grouped by 12 limbs -> integers"""
    body = text[text.index("static constexpr u32 %s(" % name):]
    body = body[body.index("{", body.index("constexpr u32 m")):body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{8})u", body)]
    assert len(words) % 12 == 0
    return [sum(w << (32 * i) for i, w in enumerate(words[k:k + 12])) for k in range(0, len(words), 12)]


def test_frobenius_constants_recomputed_from_p():
    text = open(HEADER).read()
    xi = (1, 1)

    def f2pow(a, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = bls.fp2_mul(r, r)
            if bit == "1":
                r = bls.fp2_mul(r, a)
        return r

    f1 = _table("frob1", text)
    f2 = _table("frob2", text)
    assert len(f1) == 10 and len(f2) == 5
    for i in range(1, 6):
        g = f2pow(xi, i * (P - 1) // 6)
        assert (f1[2 * (i - 1)], f1[2 * (i - 1) + 1]) == (g[0] * R % P, g[1] * R % P), i
        g2 = f2pow(xi, i * (P * P - 1) // 6)
        assert g2[1] == 0 and f2[i - 1] == g2[0] * R % P, i
    # the hard part of the final exponentiation: 3 (p^4 - p^2 + 1) / q = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3
    x = bls.BLS_X
    assert (x - 1) ** 2 * (x + P) * (x * x + P * P - 1) + 3 == 3 * (P ** 4 - P ** 2 + 1) // Q


def _fp(v):
    return (v * R % P).to_bytes(48, "little")


def g1_rec(pt):
    return b"\0" * 96 if pt is None else _fp(pt[0]) + _fp(pt[1])


def g2_rec(pt):
    return b"\0" * 192 if pt is None else b"".join(_fp(c) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]))


def gt_from_bytes(raw, i=0):
    vals = [int.from_bytes(raw[576 * i + 48 * k:576 * i + 48 * k + 48], "little") for k in range(12)]
    return tuple((vals[2 * k], vals[2 * k + 1]) for k in range(6))


def host_pairings(lib, pairs):
    a = b"".join(g1_rec(p) for p, _ in pairs)
    b = b"".join(g2_rec(q) for _, q in pairs)
    out = ctypes.create_string_buffer(576 * len(pairs))
    lib.bh_test_pairing_host(len(pairs), a, b, out)
    return [gt_from_bytes(out.raw, i) for i in range(len(pairs))]


def pyref_pairing_cubed(p, q):
    return pyp.f12_pow(pyp.f12_pow(pyp.miller_loop(p, q), pyp._FINAL_EXP), 3)


def test_host_pairing_matches_pyref(lib):
    rnd = random.Random(7)
    g1, g2 = bls.G1.gen, bls.G2.gen
    pairs = [(g1, g2), (bls.G1.mul(g1, rnd.randrange(1, Q)), bls.G2.mul(g2, rnd.randrange(1, Q)))]
    got = host_pairings(lib, pairs + [(None, g2), (g1, None)])
    for (p, q), g in zip(pairs, got):
        assert g == pyref_pairing_cubed(p, q)
    one = pyp.F12_ONE
    assert got[2] == one and got[3] == one


def test_host_pairing_inverse_and_bilinear(lib):
    rnd = random.Random(8)
    g1, g2 = bls.G1.gen, bls.G2.gen
    a, b = rnd.randrange(1, Q), rnd.randrange(1, Q)
    pa, qb = bls.G1.mul(g1, a), bls.G2.mul(g2, b)
    e1, e2, e3 = host_pairings(lib, [(pa, qb), (bls.G1.mul(g1, a * b % Q), g2), (bls.G1.neg(pa), qb)])
    assert e1 == e2
    assert pyp.f12_mul(e1, e3) == pyp.F12_ONE
    assert e1 != pyp.F12_ONE


def test_verification_error_codes():
    from bellman_amd import errors

    with pytest.raises(errors.InvalidProof):
        errors.check_verification(9)
    with pytest.raises(errors.InvalidVerifyingKey):
        errors.check_verification(8)
    with pytest.raises(errors.InvalidPoint):
        errors.check_verification(6)
    assert issubclass(errors.InvalidProof, errors.VerificationError)
    errors.check_verification(0)


def test_verifier_entry_points_in_header():
    text = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    for name in ("bh_groth16_prepare_verifying_key", "bh_groth16_pvk_from_params", "bh_groth16_verify", "bh_groth16_batch_verify",
                 "bh_groth16_pvk_release"):
        assert name in text and name in _lib.EXPORTS
    assert "#define BH_ERR_INVALID_VERIFYING_KEY 8" in text and "#define BH_ERR_INVALID_PROOF 9" in text
