"""Integer model of the split-scalar point multiplier (bellman_amd/csrc/glv.cuh): the constants, the split k = k1 + k2
lambda, the endomorphism on the Python reference's points, and the joint ladder IN THE EXPONENT - a point of the
prime-order subgroup is [e]P for the ladder's input P, so the accumulator is an integer mod q and the model says exactly
which branch of the mixed addition every step takes (copy into an identity accumulator, equal points, opposite points,
general addition) and what the result is.  Nothing here touches the library."""

from oracle.pyref import bls12_381 as bls

P, Q = bls.P, bls.Q
Z = bls.BLS_X
LAMBDA = Z * Z - 1
MU = (1 << 256) // LAMBDA
BETA = pow(2, (P - 1) // 3, P)
BETA2 = BETA * BETA % P
# which cube root psi multiplies x by, the map that acts as [LAMBDA]: found by test_glv_cpu.py against the reference
PSI = {1: BETA2, 2: BETA}
ENTRY = {(1, 0): 1, (0, 1): LAMBDA, (1, 1): LAMBDA + 1}   # the table entry of a bit pair, as a multiple of P


def split(k):
    return k % LAMBDA, k // LAMBDA


def corner_scalars():
    lam = LAMBDA
    out = [0, 1, 2, lam - 1, lam, lam + 1, 2 * lam - 1, 2 * lam, lam * lam - 1, lam * lam, lam * (lam + 1) - 1, Q - 1,
           1 << 127, (1 << 128) - 1, 1 << 128, 1 << 254]
    for m in (1, 2, 1 << 64, lam - 1, lam, lam + 1):
        out += [k for k in (m * lam - 1, m * lam, m * lam + 1) if k < Q]
    return out


def _scale_x(group, x, c):
    return c * x % P if group == 1 else (c * x[0] % P, c * x[1] % P)


def psi(group, pt):
    return None if pt is None else (_scale_x(group, pt[0], PSI[group]), pt[1])


def table(group, pt):
    """the three nonzero entries of the joint table of an affine point, by bit pair (b1, b2)"""
    curve = bls.G1 if group == 1 else bls.G2
    other = BETA if PSI[group] == BETA2 else BETA2
    return {(1, 0): pt, (0, 1): psi(group, pt), (1, 1): curve.neg((_scale_x(group, pt[0], other), pt[1]))}


def trace(k1, k2):
    """(exponent of the result, [event per step that adds]) of the MSB-first ladder over the 128 bit pairs of (k1, k2)"""
    assert 0 <= k1 < 1 << 128 and 0 <= k2 < 1 << 128
    s, events = 0, []
    for i in range(127, -1, -1):
        s = 2 * s % Q
        pair = ((k1 >> i) & 1, (k2 >> i) & 1)
        if pair == (0, 0):
            continue
        t = ENTRY[pair]
        events.append("copy" if s == 0 else "equal" if s == t else "opposite" if s == Q - t else "add")
        s = (s + t) % Q
    assert s == (k1 + k2 * LAMBDA) % Q
    return s, events


def branch_pairs():
    """[(name, k1, k2, event)]: non-canonical pairs whose ladder meets a table entry equal or opposite to its accumulator.
    A prefix (a, b) with 2 (a + b lambda) = +-t mod q for an entry t, followed by t's bit pair; (a, b) is the canonical
    split of +-t / 2 moved by short vectors of the lattice {(x, y): x + y lambda = 0 mod q} until both halves are
    non-negative and short enough to leave room for the pair."""
    lattice = [(-LAMBDA, 1), (LAMBDA + 1, LAMBDA)]
    out = []
    for pair, t in ENTRY.items():
        for sign, event in ((1, "equal"), (-1, "opposite")):
            a0, b0 = split(sign * t * pow(2, -1, Q) % Q)
            found = None
            for i in range(-3, 4):
                for j in range(-3, 4):
                    a, b = a0 + i * lattice[0][0] + j * lattice[1][0], b0 + i * lattice[0][1] + j * lattice[1][1]
                    if a >= 0 and b >= 0 and (a or b) and max(a.bit_length(), b.bit_length()) <= 127 and found is None:
                        found = (a, b)
            if found is None:   # opposite-11: the only non-negative solutions have 128 bits, no room for the pair behind them
                assert (pair, sign) == ((1, 1), -1)
                continue
            a, b = found
            fill = 127 - max(a.bit_length(), b.bit_length())   # the bits behind the pair: a tail that keeps adding
            k1 = ((a << 1 | pair[0]) << fill) | (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A & ((1 << fill) - 1))
            k2 = ((b << 1 | pair[1]) << fill) | (0x3C3C3C3C3C3C3C3C3C3C3C3C3C3C3C3C & ((1 << fill) - 1))
            out.append(("%s-%d%d" % (event, pair[0], pair[1]), k1, k2, event))
    return out
