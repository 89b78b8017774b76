"""from_compressed / from_compressed_unchecked of the Zcash BLS12-381 encoding on Python integers: the model the
compressed-point reader (bellman_amd/csrc/point_read.hip) is tested against.  Written from the encoding rules (byte 0: bit 7
compressed, bit 6 infinity, bit 5 sort; x big-endian, G2 as c1 | c0); the subgroup test is [q] P = O by plain
double-and-add, so the model shares nothing with the endomorphism tests of the kernels."""

from oracle.pyref import bls12_381 as bls
from tests.pointgen import _fp2_sqrt, _fp_sqrt

P, Q = bls.P, bls.Q
INVALID, INFINITY = "invalid", "infinity"   # error kinds (BH_ERR_INVALID_POINT, BH_ERR_POINT_AT_INFINITY)


def from_compressed(group, data, checked=True):
    """-> ("ok", point or None for the identity) or (INVALID, None)"""
    size = 48 if group == 1 else 96
    data = bytes(data)
    assert len(data) == size
    flags = data[0] >> 5
    coords = [int.from_bytes(bytes([data[k] & (0x1F if k == 0 else 0xFF)]) + data[k + 1:k + 48], "big") for k in range(0, size, 48)]
    if not flags & 4:
        return INVALID, None
    if any(c >= P for c in coords):
        return INVALID, None
    if flags & 2:
        if flags & 1 or any(coords):
            return INVALID, None
        return "ok", None
    if group == 1:
        x = coords[0]
        y = _fp_sqrt((x * x * x + 4) % P)
        if y is None:
            return INVALID, None
        if bls._fp_lex_largest(y) != bool(flags & 1):
            y = (-y) % P
        pt, curve = (x, y), bls.G1
    else:
        x = (coords[1], coords[0])
        y = _fp2_sqrt(bls.fp2_add(bls.fp2_mul(bls.fp2_mul(x, x), x), bls.G2_B))
        if y is None:
            return INVALID, None
        if bls._fp2_lex_largest(y) != bool(flags & 1):
            y = bls.fp2_neg(y)
        pt, curve = (x, y), bls.G2
    assert curve.on_curve(pt)
    if checked and curve.mul(pt, Q) is not None:
        return INVALID, None
    return "ok", pt


def read_points(group, data, checked=True, forbid_identity=True):
    """the reader over concatenated points: ("ok", [points]) or (kind, index of the first offending point)"""
    size = 48 if group == 1 else 96
    out = []
    for i in range(len(data) // size):
        kind, pt = from_compressed(group, data[i * size:(i + 1) * size], checked)
        if kind != "ok":
            return kind, i
        if pt is None and forbid_identity:
            return INFINITY, i
        out.append(pt)
    return "ok", out


def read_proof(data):
    """Proof::read of 192 bytes: ("ok", (a, b, c)) or (kind, element index 0..2), the first bad element in the order a, b, c"""
    pts = []
    for k, (group, lo, hi) in enumerate(((1, 0, 48), (2, 48, 144), (1, 144, 192))):
        kind, pt = from_compressed(group, data[lo:hi], True)
        if kind != "ok":
            return kind, k
        if pt is None:
            return INFINITY, k
        pts.append(pt)
    return "ok", tuple(pts)


# ---- the endomorphism tests of the kernels, on integers (constants passed in: the CPU test parses them out of the header) --
Z_ABS = -bls.BLS_X


def g1_endo_in_subgroup(pt, beta):
    q = bls.G1.mul(bls.G1.mul(pt, Z_ABS), Z_ABS)
    return q is not None and (beta * pt[0] % P, pt[1]) == bls.G1.neg(q)


def g2_endo_in_subgroup(pt, cx, cy):
    q = bls.G2.mul(pt, Z_ABS)
    x, y = pt
    psi = (bls.fp2_mul((x[0], (-x[1]) % P), cx), bls.fp2_mul((y[0], (-y[1]) % P), cy))
    return q is not None and psi == bls.G2.neg(q)
