"""Exponent model of the powers-of-tau check (bh_powers_of_tau_verify, bellman_amd/csrc/ceremony.hip).  A transcript is
given by its exponents - every point is [x]G for a known x mod q - so a pairing equation e([a]G1, [b]G2) = e([c]G1, [d]G2)
becomes a b = c d mod q, and with the coefficients expanded by hashlib the model predicts the exact mask of
bh_ptau_report.failed (a chance acceptance included) and the exact sums [sum rho_i x_i]G.  Nothing here touches the
library."""

import hashlib
import struct

from oracle.pyref import bls12_381 as bls

Q = bls.Q
HEAD, TAU_G1_G2, TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2, POINTS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
VECTOR_BIT = (TAU_G1, TAU_G2, ALPHA, BETA)
DOMAIN = b"bh-ptau-rlc\0"


def coefficients(seed, v, count):
    """rho_0 .. rho_{count-1} of vector v: block j = BLAKE2s-256 keyed with the seed over DOMAIN | v (u32 LE) | j (u64 LE);
    coefficient 2j = bytes 0..15 little-endian, 2j + 1 = bytes 16..31"""
    out = []
    for j in range((count + 1) // 2):
        d = hashlib.blake2s(DOMAIN + struct.pack("<IQ", v, j), key=seed, digest_size=32).digest()
        out += [int.from_bytes(d[:16], "little"), int.from_bytes(d[16:], "little")]
    return out[:count]


def coefficient_bytes(seed, v, count):
    """the same as `count` canonical 32-byte little-endian scalars"""
    return b"".join(r.to_bytes(32, "little") for r in coefficients(seed, v, count))


class Transcript:
    """exponents of tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (lists) and of beta_g2"""

    def __init__(self, t, u, a, b, beta2):
        self.vec = [[x % Q for x in v] for v in (t, u, a, b)]
        self.beta2 = beta2 % Q

    @classmethod
    def consistent(cls, tau, alpha, beta, n1, n):
        pw = [pow(tau, i, Q) for i in range(max(n1, n))]
        return cls(pw[:n1], pw[:n], [alpha * x for x in pw[:n]], [beta * x for x in pw[:n]], beta)

    def copy(self):
        return Transcript(*[list(v) for v in self.vec], self.beta2)


def sums(tr, seed):
    """[(exponent of P(V), exponent of Q(V), a consumed record is the identity)] per vector; a vector of one point has
    empty sums"""
    out = []
    for v, x in enumerate(tr.vec):
        rho = coefficients(seed, v, len(x) - 1)
        p = sum(r * e for r, e in zip(rho, x[:-1])) % Q
        q = sum(r * e for r, e in zip(rho, x[1:])) % Q
        ident = any(r % Q and (e == 0 or f == 0) for r, e, f in zip(rho, x[:-1], x[1:]))
        out.append((p, q, ident))
    return out


def equations(tr, seed):
    """[(bit, a, b, c, d)]: the equations e([a]G1, [b]G2) = e([c]G1, [d]G2) the check evaluates, in its order"""
    t, u, a, b = tr.vec
    g1, s1, g2, s2 = t[0], t[1], u[0], u[1]
    s = sums(tr, seed)
    eqs = [(TAU_G1_G2, s1, g2, g1, s2)]
    if not s[0][2]:
        eqs.append((TAU_G1, s[0][0], s2, s[0][1], g2))
    if not s[1][2]:
        eqs.append((TAU_G2, s1, s[1][0], g1, s[1][1]))
    for v, bit in ((2, ALPHA), (3, BETA)):
        if len(tr.vec[v]) > 1 and not s[v][2]:
            eqs.append((bit, s[v][0], s2, s[v][1], g2))
    eqs.append((BETA_G2, b[0], g2, g1, tr.beta2))
    return eqs


def mask(tr, seed):
    """bh_ptau_report.failed without BH_PTAU_VALIDATE_POINTS"""
    t, u, a, b = tr.vec
    if 0 in (t[0], t[1], u[0], u[1], a[0], b[0], tr.beta2):
        return HEAD
    m = 0
    for v, (_, _, ident) in enumerate(sums(tr, seed)):
        if ident:
            m |= VECTOR_BIT[v]
    for bit, w, x, y, z in equations(tr, seed):
        if (w * x - y * z) % Q:
            m |= bit
    return m
