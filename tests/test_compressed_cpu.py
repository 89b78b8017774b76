"""The compressed-point reader without a GPU: the integer model (tests/compressed_model.py) against the writer of
oracle/pyref, the constants of bellman_amd/csrc/point_read.cuh recomputed from p, the endomorphism subgroup tests against
[q] P = O, and the host build of the square roots (bh_test_fp_sqrt_host / bh_test_fp2_sqrt_host)."""

import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bellman_amd import _lib  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests import compressed_model as cm  # noqa: E402
from tests import pointgen  # noqa: E402

P, Q = bls.P, bls.Q
R = 1 << 384
HEADER = os.path.join(ROOT, "bellman_amd", "csrc", "point_read.cuh")


def _f2pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = bls.fp2_mul(r, r)
        if bit == "1":
            r = bls.fp2_mul(r, a)
    return r


def _table(name):
    """the hex words of the constexpr table `m` inside EndoConsts::<name>, 12 limbs per Fp value (Montgomery) -> integers"""
    text = open(HEADER).read()
    body = text[text.index("static constexpr u32 %s(" % name):]
    body = body[body.index("{", body.index("constexpr u32 m")):body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{8})u", body)]
    assert len(words) % 12 == 0
    rinv = pow(R, -1, P)
    return [sum(w << (32 * i) for i, w in enumerate(words[k:k + 12])) * rinv % P for k in range(0, len(words), 12)]


def header_constants():
    (beta,), cx, cy = _table("beta"), tuple(_table("psi_cx")), tuple(_table("psi_cy"))
    return beta, cx, cy


def test_model_inverts_the_writer():
    rnd = random.Random(1)
    for group, curve, comp in ((1, bls.G1, bls.g1_compress), (2, bls.G2, bls.g2_compress)):
        seen = set()
        for _ in range(12):
            pt = curve.mul(curve.gen, rnd.randrange(1, Q))
            for q in (pt, curve.neg(pt)):   # both sort flags
                data = comp(q)
                seen.add(data[0] >> 5)
                assert cm.from_compressed(group, data) == ("ok", q)
                assert cm.from_compressed(group, data, checked=False) == ("ok", q)
        assert seen == {4, 5}
        assert cm.from_compressed(group, comp(None)) == ("ok", None)
        kind, idx = cm.read_points(group, comp(curve.gen) + comp(None))
        assert (kind, idx) == (cm.INFINITY, 1)
        assert cm.read_points(group, comp(curve.gen) + comp(None), forbid_identity=False) == ("ok", [curve.gen, None])


def test_model_decodes_the_zcash_generator():
    """the compressed G1 generator of the Zcash specification (tests/test_oracle_c_vs_pyref.py holds the same string)"""
    parts = ("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58", "6c55e83ff97a1aeffb3af00adb22c6bb")
    text = open(os.path.join(ROOT, "tests", "test_oracle_c_vs_pyref.py")).read()
    assert all(part in text for part in parts)
    assert cm.from_compressed(1, bytes.fromhex("".join(parts))) == ("ok", bls.G1_GEN)


def test_model_rules():
    g = bls.g1_compress(bls.G1_GEN)
    clear = bytes([g[0] & 0x7F]) + g[1:]
    assert cm.from_compressed(1, clear)[0] == cm.INVALID
    xp = bytearray(P.to_bytes(48, "big"))
    xp[0] |= 0x80
    assert cm.from_compressed(1, bytes(xp))[0] == cm.INVALID
    assert cm.from_compressed(1, bytes([0xE0]) + bytes(47))[0] == cm.INVALID            # infinity + sort
    assert cm.from_compressed(1, bytes([0xC0]) + bytes(46) + b"\x01")[0] == cm.INVALID   # infinity + a stray bit
    t = pointgen.g1_on_curve_not_in_subgroup(5)
    assert cm.from_compressed(1, bls.g1_compress(t))[0] == cm.INVALID
    assert cm.from_compressed(1, bls.g1_compress(t), checked=False) == ("ok", t)
    flipped = bytes([g[0] ^ 0x20]) + g[1:]
    assert cm.from_compressed(1, flipped) == ("ok", bls.G1.neg(bls.G1_GEN))


def test_header_constants_recomputed_from_p():
    beta, cx, cy = header_constants()
    assert beta == pow(2, (P - 1) // 3, P) and beta != 1 and pow(beta, 3, P) == 1
    assert cx == bls.fp2_inv(_f2pow((1, 1), (P - 1) // 3))
    assert cy == bls.fp2_inv(_f2pow((1, 1), (P - 1) // 2))
    text = open(HEADER).read()
    assert "0xd201000000010000ull" in text and cm.Z_ABS == 0xD201000000010000
    # the curve order in terms of the parameter: the relation both tests rest on
    z = bls.BLS_X
    assert z ** 4 - z ** 2 + 1 == Q and (z - 1) ** 2 * Q // 3 + z == P


def _non_subgroup(group, rnd):
    """>= 8 points on the curve outside the subgroup: random curve points, pure cofactor torsion, subgroup + torsion sums"""
    curve = bls.G1 if group == 1 else bls.G2
    gen = pointgen.g1_on_curve_not_in_subgroup if group == 1 else pointgen.g2_on_curve_not_in_subgroup
    out = []
    for s in range(3):
        t = gen(1000 + 37 * s)
        tors = curve.mul(t, Q)                       # order divides the cofactor
        assert tors is not None and curve.on_curve(tors)
        out += [t, tors, curve.add(tors, curve.mul(curve.gen, rnd.randrange(1, Q)))]
    if group == 1:
        assert bls.G1.mul((0, 2), 3) is None         # a point of order 3
        out += [(0, 2), bls.G1.add((0, 2), bls.G1.mul(bls.G1.gen, 12345))]
    return out


@pytest.mark.parametrize("group", [1, 2])
def test_endomorphism_tests_agree_with_q_multiplication(group):
    beta, cx, cy = header_constants()
    curve = bls.G1 if group == 1 else bls.G2
    test = (lambda p: cm.g1_endo_in_subgroup(p, beta)) if group == 1 else (lambda p: cm.g2_endo_in_subgroup(p, cx, cy))
    rnd = random.Random(40 + group)
    inside = [curve.gen, curve.neg(curve.gen)] + [curve.mul(curve.gen, rnd.randrange(1, Q)) for _ in range(7)]
    outside = _non_subgroup(group, rnd)
    assert len(inside) >= 8 and len(outside) >= 8
    for p in inside:
        assert curve.mul(p, Q) is None and test(p)
    for p in outside:
        assert curve.on_curve(p) and curve.mul(p, Q) is not None and not test(p)
    if group == 1:   # the other cube root of unity fails for subgroup points
        assert not cm.g1_endo_in_subgroup(inside[3], beta * beta % P)


# ---- host build of the square roots ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.TEST_LIB_PATH):
        _lib.build()
    return _lib.load()


def _mont(v):
    return (v * R % P).to_bytes(48, "little")


def _unmont(raw):
    return int.from_bytes(raw, "little") * pow(R, -1, P) % P


def test_host_fp_sqrt(lib):
    rnd = random.Random(3)
    vals = [0, 1, P - 1, 4, 2, (P - 1) // 2] + [rnd.randrange(P) for _ in range(60)] + [pow(rnd.randrange(P), 2, P) for _ in range(20)]
    a = b"".join(_mont(v) for v in vals)
    out, ok = ctypes.create_string_buffer(48 * len(vals)), ctypes.create_string_buffer(len(vals))
    lib.bh_test_fp_sqrt_host(out, ok, a, len(vals))
    kinds = set()
    for i, v in enumerate(vals):
        want = pointgen._fp_sqrt(v)
        kinds.add(want is None)
        assert (ok.raw[i] == 1) == (want is not None), v
        if want is not None:
            r = _unmont(out.raw[48 * i:48 * i + 48])
            assert r * r % P == v and r in (want, P - want)
    assert kinds == {True, False}


def test_host_fp2_sqrt(lib):
    rnd = random.Random(4)
    vals = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (4, 4)]
    vals += [(rnd.randrange(P), 0) for _ in range(12)]                        # c1 = 0: squares and non-squares of Fp
    vals += [(rnd.randrange(P), rnd.randrange(P)) for _ in range(50)]
    vals += [bls.fp2_mul(v, v) for v in [(rnd.randrange(P), rnd.randrange(P)) for _ in range(20)]]
    a = b"".join(_mont(v[0]) + _mont(v[1]) for v in vals)
    out, ok = ctypes.create_string_buffer(96 * len(vals)), ctypes.create_string_buffer(len(vals))
    lib.bh_test_fp2_sqrt_host(out, ok, a, len(vals))
    kinds = set()
    for i, v in enumerate(vals):
        want = pointgen._fp2_sqrt(v)
        kinds.add(want is None)
        assert (ok.raw[i] == 1) == (want is not None), v
        if want is not None:
            r = (_unmont(out.raw[96 * i:96 * i + 48]), _unmont(out.raw[96 * i + 48:96 * i + 96]))
            assert bls.fp2_mul(r, r) == v, v
    assert kinds == {True, False}


def test_new_entry_points_in_header_and_exports():
    text = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    for name in ("bh_bases_read_compressed", "bh_proofs_read", "bh_groth16_batch_verify_compressed"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.EXPORTS
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert "stays with the caller" in text and "bh_proofs_read and" in text


def test_python_readers_report_short_input():
    from bellman_amd import UnexpectedEof
    from bellman_amd import groth16 as pg

    with pytest.raises(UnexpectedEof):
        pg.Proof.read(None, bytes(191))
    with pytest.raises(UnexpectedEof):
        pg.read_proofs(None, bytes(193))
