"""Exponent model of the ceremony-step check (bh_groth16_params_verify_step, bh_pairing_same_ratio_each and the Python
helpers of bellman_amd/ceremony.py).  A parameter set is a tuple of integers mod q - every point is [x]G for a known x -
so byte equality of records becomes equality of exponents, a pairing equation e([a]G1, [b]G2) = e([c]G1, [d]G2) becomes
a b = c d mod q, and with the coefficients expanded by hashlib (tags 4 and 5 of ptau_verify_model.coefficients) the model
predicts the exact mask, bad_vector and bad_index of bh_params_step_report, the exact four sums, and every verdict of
bh_pairing_same_ratio_each.  OFF stands for a record that is not on its curve.  Nothing here touches the library."""

import collections

from tests.models import ptau_verify_model as ptau

Q = ptau.Q
SHAPE, HEAD, KEY, A, B_G1, B_G2, DELTA, H, L, POINTS = (1 << i for i in range(10))
TAG_H, TAG_L = 4, 5
OFF = "off-curve"
OK, INVALID_POINT, POINT_AT_INFINITY, INVALID_TRANSCRIPT = 0, 6, 7, 10

# exponents: alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2 (numbers), ic, h, l, a, b_g1, b_g2 (tuples)
Params = collections.namedtuple("Params", "alpha_g1 beta_g1 beta_g2 gamma_g2 delta_g1 delta_g2 ic h l a b_g1 b_g2")


def rescale_delta(p, d):
    """the honest step: delta *= d, h and l *= 1/d"""
    inv = pow(d, -1, Q)
    return p._replace(delta_g1=p.delta_g1 * d % Q, delta_g2=p.delta_g2 * d % Q, h=tuple(x * inv % Q for x in p.h),
                      l=tuple(x * inv % Q for x in p.l))


def sums(before, after, seed):
    """[(exponent, a consumed record is the identity)] for sum rho_i h_i, sum rho_i h'_i (tag 4), sum rho_i l_i,
    sum rho_i l'_i (tag 5); an empty query has the empty sum 0"""
    out = []
    for tag, x, y in ((TAG_H, before.h, after.h), (TAG_L, before.l, after.l)):
        rho = ptau.coefficients(seed, tag, len(x))
        for v in (x, y):
            out.append((sum(r * e for r, e in zip(rho, v)) % Q, any(r % Q and e % Q == 0 for r, e in zip(rho, v))))
    return out


def _first_difference(x, y):
    for i, (u, v) in enumerate(zip(x, y)):
        if u != v and (u is OFF or v is OFF or (u - v) % Q):
            return i
    return len(x)


def step(before, after, seed, bad_points=None):
    """(failed, bad_vector, bad_index) of bh_groth16_params_verify_step.  bad_points: what BH_STEP_VALIDATE_POINTS would
    find, as (vector 4..7, index) of the first point of `after` outside the subgroup or equal to the identity in the order
    h, l, delta_g1, delta_g2 - None without the flag or when every point is good (identities in h and l are found by the
    model itself)."""
    if len(before.ic) != len(after.ic) or any(len(getattr(before, q)) != len(getattr(after, q)) for q in ("h", "l", "a", "b_g1", "b_g2")):
        return SHAPE, 0, 0
    deltas = (before.delta_g1, after.delta_g1, before.delta_g2, after.delta_g2)
    if any(x is OFF or x % Q == 0 for x in deltas):
        return HEAD, 0, 0
    if bad_points is not None:
        return POINTS, bad_points[0], bad_points[1]
    failed, placed = 0, None
    key_b = (before.alpha_g1, before.beta_g1, before.beta_g2, before.gamma_g2) + tuple(before.ic)
    key_a = (after.alpha_g1, after.beta_g1, after.beta_g2, after.gamma_g2) + tuple(after.ic)
    at = _first_difference(key_b, key_a)
    if at != len(key_b):
        failed, placed = failed | KEY, (0, at)
    for vector, (bit, name) in enumerate(((A, "a"), (B_G1, "b_g1"), (B_G2, "b_g2")), start=1):
        at = _first_difference(getattr(before, name), getattr(after, name))
        if at != len(getattr(before, name)):
            failed |= bit
            placed = placed or (vector, at)
    if (after.delta_g1 * before.delta_g2 - before.delta_g1 * after.delta_g2) % Q:
        failed |= DELTA
    s = sums(before, after, seed)
    for bit, k, n in ((H, 0, len(before.h)), (L, 2, len(before.l))):
        if s[k][1] or s[k + 1][1]:
            failed |= bit
        elif n and (s[k][0] * before.delta_g2 - s[k + 1][0] * after.delta_g2) % Q:
            failed |= bit
    return (failed,) + (placed or (0, 0))


def validation_finding(after):
    """(vector, index) of the first identity among h', l' in that order - what BH_STEP_VALIDATE_POINTS reports for a set whose
    points are otherwise all of the form [x]G - or None"""
    for vector, v in ((4, after.h), (5, after.l)):
        for i, x in enumerate(v):
            if x % Q == 0:
                return vector, i
    return None


def same_ratio(rows):
    """the verdicts of bh_pairing_same_ratio_each for rows (a, b, A, B) of exponents (0 the identity, OFF off the curve):
    e([a]G1, [B]G2) == e([b]G1, [A]G2)"""
    out = []
    for row in rows:
        if any(x is not OFF and x % Q == 0 for x in row):
            out.append(POINT_AT_INFINITY)
        elif any(x is OFF for x in row):
            out.append(INVALID_POINT)
        else:
            a, b, A_, B_ = row
            out.append(OK if (a * B_ - b * A_) % Q == 0 else INVALID_TRANSCRIPT)
    return out


def contribution(delta_before, d, s, r):
    """(exponents of) what ceremony.contribute returns beside the parameters: delta_g1_after, s, [d]s, [d]r"""
    return (delta_before * d % Q, s % Q, s * d % Q, r * d % Q)


def contributions(delta_first, contribs, challenges):
    """the verdict list of ceremony.verify_contributions: two rows per contribution, the first nonzero code of the two"""
    rows, prev = [], delta_first
    for (delta_after, s, ds, dr), r in zip(contribs, challenges):
        rows += [(s, ds, r, dr), (prev, delta_after, r, dr)]
        prev = delta_after
    v = same_ratio(rows)
    return [v[2 * j] or v[2 * j + 1] for j in range(len(contribs))]
