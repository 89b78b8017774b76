"""Rows for the tests of the device proof assembly (csrc/proof_finish.cuh): a verifying key, eight multiexp sums and a
blinding pair per row, every point a KNOWN multiple of its group's generator - so the proof the row must give is three
integers mod q (prover.rs:326-360 on discrete logarithms), and a corner (an identity element, an addition that meets its own
operand or its negative) is an equation between exponents.  The key is tests/pointgen.py's."""

import random

import numpy as np

from oracle import cref
from oracle.pyref import bls12_381 as bls
from tests import pointgen
from tests.models import glv_model

Q, LAM = bls.Q, glv_model.LAMBDA
SLOTS = ("a_in", "a_aux", "b1_in", "b1_aux", "b2_in", "b2_aux", "h", "l")   # BH_MSM_SUMS_BYTES' order
GROUP = dict(a_in=1, a_aux=1, b1_in=1, b1_aux=1, b2_in=2, b2_aux=2, h=1, l=1)
# the multiples pointgen.small_parameters() (k0 = 11) takes for the key: +7 per G1 point, +5 per G2 point, in its order
KEY = dict(alpha_g1=18, beta_g1=25, beta_g2=30, delta_g1=42, delta_g2=47)
KEY_GROUP = dict(alpha_g1=1, beta_g1=1, beta_g2=2, delta_g1=1, delta_g2=2)


def point(group, e):
    """[e] G as a Montgomery record (uint64[12] / [24]); e = 0 mod q: the identity, the all-zero record"""
    gen = cref.g1_generator() if group == 1 else cref.g2_generator()
    e %= Q
    return cref.point_mul(group, gen, e) if e else np.zeros(12 * group, dtype=np.uint64)


def key_points():
    """pointgen's verifying key as Python points, checked against KEY's multiples"""
    vk = pointgen.small_parameters()[0]
    for name, e in KEY.items():
        curve = bls.G1 if KEY_GROUP[name] == 1 else bls.G2
        assert vk[name] == curve.mul(curve.gen, e), name
    return vk


def key_records(key=None):
    key = key or KEY
    return {name: point(KEY_GROUP[name], e) for name, e in key.items()}


def vk5(key=None):
    """alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2: BH_FINISH_KEY_BYTES"""
    rec = key_records(key)
    return np.concatenate([rec[n] for n in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")])


def proof_exponents(row, key=None):
    """(A, B, C) of prover.rs:326-360 as multiples of the generators"""
    k = key or KEY
    r, s, e = row["r"], row["s"], row["sums"]
    a = k["alpha_g1"] + r * k["delta_g1"] + e["a_in"] + e["a_aux"]
    b = k["beta_g2"] + s * k["delta_g2"] + e["b2_in"] + e["b2_aux"]
    c = (r * s * k["delta_g1"] + s * k["alpha_g1"] + r * k["beta_g1"] + s * (e["a_in"] + e["a_aux"]) +
         r * (e["b1_in"] + e["b1_aux"]) + e["h"] + e["l"])
    return a % Q, b % Q, c % Q


def corner_rows():
    """name -> row; the names say which branch or identity the row is there for"""
    rnd = random.Random(0x9F1)
    a1, d1, b2, d2 = KEY["alpha_g1"], KEY["delta_g1"], KEY["beta_g2"], KEY["delta_g2"]
    inv = lambda x: pow(x, -1, Q)  # noqa: E731

    def row(r=None, s=None, **sums):
        e = {n: rnd.randrange(1, Q) for n in SLOTS}
        e.update(sums)
        return dict(r=rnd.randrange(1, Q) if r is None else r, s=rnd.randrange(1, Q) if s is None else s, sums=e)

    rows = {
        "r-zero": row(r=0), "s-zero": row(s=0), "both-zero": row(r=0, s=0),
        "r-q-minus-1": row(r=Q - 1), "s-q-minus-1": row(s=Q - 1),
        "r-low-half-zero": row(r=rnd.randrange(1, LAM) * LAM), "s-high-half-zero": row(s=rnd.randrange(1, LAM)),
        "rs-is-one": None, "all-sums-identity": row(**{n: 0 for n in SLOTS}),
        "h-is-minus-l": row(h=5, l=Q - 5), "h-l-identity": row(h=0, l=0),
    }
    r = rnd.randrange(2, Q)
    rows["rs-is-one"] = row(r=r, s=inv(r))
    x = rnd.randrange(1, Q)
    rows["a-in-equals-a-aux"] = row(a_in=x, a_aux=x)
    rows["a-in-is-minus-a-aux"] = row(a_in=x, a_aux=Q - x)
    rows["b2-in-equals-b2-aux"] = row(b2_in=x, b2_aux=x)
    rows["b1-in-is-minus-b1-aux"] = row(b1_in=x, b1_aux=Q - x)
    # ONE identity among an element's sums: adding the all-zero record as if it were a point is an involution on the running
    # sum, so two identities in a row (or one behind an identity running sum) would hide a missing identity case
    rows["a-aux-alone-identity"] = row(a_aux=0)
    rows["a-in-alone-identity"] = row(a_in=0)
    rows["b2-in-alone-identity"] = row(b2_in=0)
    rows["b2-aux-alone-identity"] = row(b2_aux=0)
    rows["h-alone-identity"] = row(h=0)
    rows["l-alone-identity"] = row(l=0)
    r, s = rnd.randrange(1, Q), rnd.randrange(1, Q)
    rows["A-identity"] = row(r=r, a_in=-(a1 + r * d1) % Q, a_aux=0)           # a_in = -(alpha + [r] delta)
    rows["B-identity"] = row(s=s, b2_in=-(b2 + s * d2) % Q, b2_aux=0)
    rows["A-doubles-on-a-aux"] = row(r=r, a_in=x, a_aux=(a1 + r * d1 + x) % Q)   # the running sum meets the point it adds
    rows["B-doubles-on-b2-in"] = row(s=s, b2_in=(b2 + s * d2) % Q)
    rows["A-doubles-on-alpha"] = row(r=inv(d1) * a1 % Q)                      # [r] delta = alpha
    rows["A-cancels-on-alpha"] = row(r=-inv(d1) * a1 % Q)                     # [r] delta = -alpha; C: [rs] delta = -[s] alpha
    rows["B-cancels-on-beta"] = row(s=-inv(d2) * b2 % Q)
    full = row()
    a, _, c = proof_exponents(full)
    rows["C-identity"] = row(r=full["r"], s=full["s"], **dict(full["sums"], l=(full["sums"]["l"] - c) % Q))
    rows["C-doubles-on-h"] = row(r=full["r"], s=full["s"], **dict(full["sums"], l=0, h=(c - full["sums"]["l"] - full["sums"]["h"]) % Q))
    assert proof_exponents(rows["A-identity"])[0] == 0 and proof_exponents(rows["B-identity"])[1] == 0
    assert proof_exponents(rows["C-identity"])[2] == 0
    return rows


def random_rows(n, seed):
    rnd = random.Random(seed)
    return [dict(r=rnd.randrange(Q), s=rnd.randrange(Q), sums={name: rnd.randrange(Q) for name in SLOTS}) for _ in range(n)]


_cache = {}


def sums_record(row):
    """the row's BH_MSM_SUMS_BYTES record, uint64[120]"""
    out = []
    for name in SLOTS:
        key = (GROUP[name], row["sums"][name] % Q)
        if key not in _cache:
            _cache[key] = point(*key)
        out.append(_cache[key])
    return np.concatenate(out)


def expected_proof(row, key=None):
    """the 384-byte record from the exponents: uint64[48]"""
    a, b, c = proof_exponents(row, key)
    return np.concatenate([point(1, a), point(2, b), point(1, c)])
