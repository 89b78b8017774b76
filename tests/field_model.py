"""Fp, Fr, Fp2, Fp6 and Fp12 of BLS12-381 on Python integers: the plain reference the field-level tests compare the HIP
field arithmetic with (tests/test_field_model_cpu.py pins it, tests/test_gpu_field_corners.py uses it), the corner
operand tables both tests share, and the expectations for every form x operation of bh_test_field_ops_dev / _host.

Tower as in csrc/fp12.cuh:  Fp2 = Fp[u]/(u^2 + 1),  Fp6 = Fp2[v]/(v^3 - xi) with xi = u + 1,  Fp12 = Fp6[w]/(w^2 - v).
Values: Fp an int, Fp2 (c0, c1), Fp6 (a, b, c), Fp12 (c0, c1) - the memory order of fp2_t / fp6_t / fp12_t.  Frobenius is
x -> x^p by `pow`, square roots are exponentiations.  Montgomery factors: R = 2^384 (Fp), 2^256 (Fr).  Nothing here calls
oracle/c; only the two moduli and the curve parameter come from oracle/pyref."""

import ctypes
import random

import numpy as np

from oracle.pyref import bls12_381 as bls

P, Q = bls.P, bls.Q
RP, RQ = 1 << 384, 1 << 256
RP_INV, RQ_INV = pow(RP, -1, P), pow(RQ, -1, Q)
X_ABS = -bls.BLS_X
ONES = RP - 1


# ------------------------------------------------------------------------------------------------------------ the fields
def fp_inv(a):
    return pow(a, P - 2, P)


def fp_is_square(a):
    return a % P == 0 or pow(a, (P - 1) // 2, P) == 1


def fp_sqrt(a):
    """a root of a (p = 3 mod 4: a^((p + 1) / 4)), None when a is not a square"""
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


F2_ZERO, F2_ONE, XI = (0, 0), (1, 0), (1, 1)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2_conj(a):
    return (a[0] % P, -a[1] % P)


def f2_inv(a):
    """0 -> 0 (what x^(p^2 - 2) gives)"""
    n = fp_inv((a[0] * a[0] + a[1] * a[1]) % P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r = F2_ONE
    for bit in bin(e)[2:]:
        r = f2_mul(r, r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


def f2_is_square(a):
    """the norm test: a is a square in Fp2 exactly when a0^2 + a1^2 is one in Fp"""
    return fp_is_square((a[0] * a[0] + a[1] * a[1]) % P)


def f2_sqrt(a):
    """by exponentiation (p = 3 mod 4; Adj, Rodriguez-Henriquez, "Square root computation over even extension fields",
    algorithm 9); None when a is not a square"""
    a = (a[0] % P, a[1] % P)
    if a == F2_ZERO:
        return F2_ZERO
    a1 = f2_pow(a, (P - 3) // 4)
    alpha = f2_mul(f2_mul(a1, a1), a)
    a0 = f2_mul(f2_pow(alpha, P), alpha)
    if a0 == (P - 1, 0):
        return None
    x0 = f2_mul(a1, a)
    if alpha == (P - 1, 0):
        return f2_mul((0, 1), x0)
    return f2_mul(f2_pow(f2_add(F2_ONE, alpha), (P - 1) // 2), x0)


F6_ZERO = (F2_ZERO,) * 3
F6_ONE = (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    """schoolbook in v, reduced with v^3 = xi"""
    acc = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            acc[i + j] = f2_add(acc[i + j], f2_mul(a[i], b[j]))
    return (f2_add(acc[0], f2_mul(acc[3], XI)), f2_add(acc[1], f2_mul(acc[4], XI)), acc[2])


def f6_mul_v(a):
    return (f2_mul(a[2], XI), a[0], a[1])


def f6_inv(a):
    """by the adjoint: a^-1 = (t0, t1, t2) / (a0 t0 + xi (a2 t1 + a1 t2)); 0 -> 0"""
    t0 = f2_sub(f2_mul(a[0], a[0]), f2_mul(XI, f2_mul(a[1], a[2])))
    t1 = f2_sub(f2_mul(XI, f2_mul(a[2], a[2])), f2_mul(a[0], a[1]))
    t2 = f2_sub(f2_mul(a[1], a[1]), f2_mul(a[0], a[2]))
    d = f2_add(f2_mul(a[0], t0), f2_mul(XI, f2_add(f2_mul(a[2], t1), f2_mul(a[1], t2))))
    d = f2_inv(d)
    return (f2_mul(t0, d), f2_mul(t1, d), f2_mul(t2, d))


F12_ZERO = (F6_ZERO, F6_ZERO)
F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    """(a0 + a1 w)(b0 + b1 w) with w^2 = v"""
    return (f6_add(f6_mul(a[0], b[0]), f6_mul_v(f6_mul(a[1], b[1]))), f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_conj(a):
    return (tuple(f2_add(x, F2_ZERO) for x in a[0]), f6_neg(a[1]))


def f12_inv(a):
    d = f6_inv(f6_sub(f6_mul(a[0], a[0]), f6_mul_v(f6_mul(a[1], a[1]))))
    return (f6_mul(a[0], d), f6_neg(f6_mul(a[1], d)))


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_frob(a, k=1):
    return f12_pow(a, P ** k)


def f12_cyclotomic(f):
    """the easy part of the final exponentiation, f^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup"""
    m = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_frob(m, 2), m)


FINAL_EXP = 3 * (P ** 12 - 1) // Q    # what f12_final_exp computes (csrc/fp12.cuh)


def f12_to_wbasis(a):
    """coefficients of w^0 .. w^5 (oracle/pyref/pairing.py's representation)"""
    return tuple(a[k & 1][k >> 1] for k in range(6))


def f12_from_wbasis(g):
    return ((g[0], g[2], g[4]), (g[1], g[3], g[5]))


def flat(x):
    """the Fp coefficients of a value in memory order"""
    return [x] if isinstance(x, int) else [c for e in x for c in flat(e)]


def shaped(like, coeffs):
    """the inverse of flat: a value with the nesting of `like` from an iterator of Fp coefficients"""
    return next(coeffs) if isinstance(like, int) else tuple(shaped(e, coeffs) for e in like)


def fmap(f, x):
    return f(x) if isinstance(x, int) else tuple(fmap(f, e) for e in x)


def real(x):
    """Montgomery residue(s) in any representative -> the value(s) in [0, p)"""
    return fmap(lambda v: v * RP_INV % P, x)


def mont(x):
    return fmap(lambda v: v * RP % P, x)


# ------------------------------------------------------------------------------------------------------- operand tables
def _dedupe(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _limb_patterns(bound):
    """the largest values below `bound` whose 30-bit limbs are all 0x3fffffff as far up as the bound allows, and whose
    32-bit limbs alternate 0xffffffff / 0 (both phases)"""

    def cap(v, limb_bits):
        if v < bound:
            return v
        s = limb_bits * ((v.bit_length() - 1) // limb_bits)        # where the top limb starts
        v = ((bound - 1) >> s << s) | (v & ((1 << s) - 1))         # the bound's own top limb ...
        return v if v < bound else v - (1 << s)                    # ... or one less

    top = bound - 1
    out = [cap((1 << (30 * ((top.bit_length() + 29) // 30))) - 1, 30)]
    for phase in (0, 1):
        out.append(cap(sum(0xFFFFFFFF << (32 * i) for i in range(phase, (top.bit_length() + 31) // 32, 2)), 32))
    return out


def corner_values(m, rbits, bound):
    """the corner table of one prime field: modulus m, Montgomery factor 2^rbits, values below `bound` (m for the canonical
    forms, 2m for the lazily reduced ones)"""
    r = (1 << rbits) % m
    vals = [0, 1, 2, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1]
    vals += [r, r - 1, r + 1, (m + 1) // 2, (m - 1) // 2, (m - 3) // 4]
    ks = sorted({k + d for step in (30, 32) for k in range(step, rbits, step) for d in (-1, 0, 1)})
    for k in ks:
        vals += [1 << k, (1 << k) - 1]
    vals += _limb_patterns(bound)
    return [v for v in _dedupe(vals) if 0 <= v < bound]


FP_LAZY = corner_values(P, 384, 2 * P)            # [0, 2p)
FP_CANON = corner_values(P, 384, P)
FR_CANON = corner_values(Q, 256, Q)
# any 384-bit word may enter the Fp multiplier (the words of test_abi_cpu's maximal-limb test, and 2p itself: what the
# fused product is fed for c = 0)
FP_WIDE = [ONES, ONES >> 1, (1 << 383) - 1, (1 << 382) - 1, 2 * P, int("3fffffff" * 13, 16) & ONES, (1 << 381) | ((1 << 381) - 1)]
FR_WIDE = [RQ - 1, (RQ - 1) >> 1, 2 * Q - 1, 2 * Q, int("3fffffff" * 9, 16) & (RQ - 1), Q + 1]
# a short list for the places where a full cross product of FP_LAZY would be too large (quadruples, Fp2 x Fp2)
FP_CORE = [0, 1, P - 1, P, P + 1, 2 * P - 2, 2 * P - 1, RP % P, (P - 1) // 2, (P + 1) // 2, FP_LAZY[-3], FP_LAZY[-2], FP_LAZY[-1],
           (1 << 360) - 1, 1 << 30]
N_RANDOM = 4000


def _rng(tag):
    return random.Random("field corners " + tag)


def unary_table(corners, bound, tag, n_random=N_RANDOM):
    rnd = _rng(tag)
    return list(corners) + [rnd.randrange(bound) for _ in range(n_random)]


def binary_table(corners, m, bound, tag, n_random=N_RANDOM):
    """the cross product of the corners, the pairs built for the branches of add / sub / eq, and seeded random pairs"""
    rnd = _rng(tag)
    pairs = [(a, b) for a in corners for b in corners]
    if bound == 2 * m:
        for x in [c for c in corners if 2 <= c < 2 * m - 2]:
            pairs += [(x, 2 * m - x), (x, 2 * m - 1 - x), (x, 2 * m + 1 - x)]       # a + b = 2p, 2p - 1, 2p + 1
        for x in [c for c in corners if c < m]:
            pairs += [(x, x + m), (x + m, x)]                                      # a - b = 0, different representatives
    else:
        for x in [c for c in corners if 2 <= c < m - 2]:
            pairs += [(x, m - x), (x, m - 1 - x), (x, m + 1 - x)]                   # a + b = m, m - 1, m + 1
    pairs += [(x, x + 1) for x in corners if x + 1 < bound]                         # a - b = -1
    pairs += [(rnd.randrange(bound), rnd.randrange(bound)) for _ in range(n_random)]
    assert all(0 <= a < bound and 0 <= b < bound for a, b in pairs)
    return pairs


def high_limb_values(bound, n, tag):
    """seeded values below `bound` whose 30-bit limbs are ALL within 2^8 of 0x3fffffff, as far up as the bound allows.  The
    compile-time column plans of csrc/ff.cuh (Radix30::NOSPLIT, Radix30Fused::PLAN) are proved with every limb of every
    operand at 2^30 - 1; a middle column of the reduction only comes near 2^64 for operands of this kind, and whether it
    passes depends on the quotient digits, which the low bits vary."""
    rnd = _rng("high limbs " + tag)
    out = []
    for _ in range(n):
        v = sum((0x3FFFFFFF - rnd.randrange(256)) << (30 * i) for i in range(13)) & ONES
        while v >= bound:
            v -= 1 << (v.bit_length() - 1)
        out.append(v)
    return out


HIGH_WIDE = high_limb_values(RP, 60, "wide")
HIGH_LAZY = high_limb_values(2 * P, 60, "lazy")


def product_table(tag):
    """binary_table of the lazy Fp domain plus every wide word against every value of the domain, either way round: the
    product stays below 2^384 (w b / 2^384 + p < 3p)"""
    pairs = binary_table(FP_LAZY, P, 2 * P, tag)
    pairs += [(w, c) for w in FP_WIDE for c in FP_LAZY] + [(c, w) for w in FP_WIDE for c in FP_LAZY]
    pairs += [(a, b) for a in HIGH_WIDE for b in HIGH_LAZY] + [(b, a) for a in HIGH_WIDE[:20] for b in HIGH_LAZY[:20]]
    assert all(a * b // RP + P < RP for a, b in pairs)
    return pairs


def fp_quad_table():
    """mul2_sub(a, b, c, d) = a b - c d: c = 0 (the multiplier is fed 2p), c = p, a b = c d in several representatives, all
    four operands at 2p - 1, every quadruple of the short corner list's first eight, and seeded random quadruples"""
    rnd = _rng("fp quads")
    quads = []
    for a in FP_CORE:
        for b in FP_CORE:
            quads += [(a, b, 0, b), (a, b, P, a), (a, b, 0, 0), (a, b, a, b), (a, b, b, a), (a, b, (a + P) % (2 * P), b),
                      (a, b, 2 * P - 1, 2 * P - 1)]
    quads.append((2 * P - 1,) * 4)
    core8 = FP_CORE[:8]
    quads += [(a, b, c, d) for a in core8 for b in core8 for c in core8 for d in core8]
    for x in FP_LAZY:
        y = FP_LAZY[(FP_LAZY.index(x) * 7 + 3) % len(FP_LAZY)]
        quads += [(x, y, 0, x), (x, y, y, x), (x, x, y, y)]
    # every limb of all four multiplier inputs near its maximum: c = 2p - h feeds the multiplier h
    h = HIGH_LAZY
    quads += [(h[i], h[(i + j) % 60], 2 * P - h[(i + 2 * j) % 60], h[(i + 3 * j) % 60]) for i in range(60) for j in range(1, 11)]
    quads += [tuple(rnd.randrange(2 * P) for _ in range(4)) for _ in range(3000)]
    return quads


def fp2_unary_table(n_random=2000):
    """all pairs of Fp corners - (x, 0), (0, x), (p, p), (x, x) among them - then (x, p - x), then random values"""
    rnd = _rng("fp2 unary")
    vals = [(a, b) for a in FP_LAZY for b in FP_LAZY]
    vals += [(x, P - x) for x in FP_LAZY if x <= P] + [(x, 2 * P - x) for x in FP_LAZY if 0 < x]
    vals += [(rnd.randrange(2 * P), rnd.randrange(2 * P)) for _ in range(n_random)]
    return vals


FP2_CORE = [(a, b) for a in FP_CORE for b in FP_CORE] + [(x, P - x) for x in FP_CORE if x <= P]


def fp2_binary_table(n_random=3000):
    rnd = _rng("fp2 binary")
    r2 = lambda: (rnd.randrange(2 * P), rnd.randrange(2 * P))   # noqa: E731
    pairs = [(a, b) for a in FP2_CORE for b in FP2_CORE]
    pairs += [(a, ((a[0] + P) % (2 * P), a[1])) for a in FP2_CORE] + [(a, (a[0], (a[1] + P) % (2 * P))) for a in FP2_CORE]
    full = fp2_unary_table(0)
    pairs += [(a, full[(i * 37 + 11) % len(full)]) for i, a in enumerate(full)]      # every pair of Fp corners appears once
    pairs += [(r2(), r2()) for _ in range(n_random)]
    return pairs


def fp2_quad_table():
    rnd = _rng("fp2 quads")
    r2 = lambda: (rnd.randrange(2 * P), rnd.randrange(2 * P))   # noqa: E731
    c = FP2_CORE
    quads = []
    for i, a in enumerate(c):
        b, d = c[(i * 5 + 1) % len(c)], c[(i * 11 + 7) % len(c)]
        quads += [(a, b, (0, 0), d), (a, b, (P, P), d), (a, b, a, b), (a, b, b, a), (a, b, d, a), (a, a, a, a)]
    quads.append(((2 * P - 1, 2 * P - 1),) * 4)
    quads += [(r2(), r2(), r2(), r2()) for _ in range(2000)]
    return quads


LANE_KEYS = [(0, 0), (P, P), (0, P), (2 * P - 1, 2 * P - 1), (RP % P, 0), (FP_LAZY[-3], FP_LAZY[-3]), (P - 1, 1)]


def lane_layout(table, tag, arity):
    """Operands for the lane-triple / lane-pair forms: corner elements and random ones alternate, so they share
    wavefronts and the corners land on every lane position; each key element also runs 67 times in a row (every one of
    the 21 triple and 32 pair positions of a wavefront, across a wavefront boundary); the length is no multiple of 21 or
    of 32, so the last wavefront is ragged."""
    rnd = _rng("lanes " + tag)
    r2 = lambda: (rnd.randrange(2 * P), rnd.randrange(2 * P))   # noqa: E731
    out = []
    for i, e in enumerate(table):
        out.append(e)
        if i % 2:
            out.append(r2() if arity == 1 else tuple(r2() for _ in range(arity)))
    for k in LANE_KEYS:
        for j in range(67):
            out.append(k if arity == 1 else (k,) + tuple(LANE_KEYS[(j + t) % len(LANE_KEYS)] for t in range(1, arity)))
    while len(out) % 21 == 0 or len(out) % 32 == 0:
        out.append(r2() if arity == 1 else tuple(r2() for _ in range(arity)))
    return out


# ---- tower operands ---------------------------------------------------------------------------------------------------
def _rand_flat(rnd, n, bound=None):
    return [rnd.randrange(bound or 2 * P) for _ in range(n)]


def tower_values(width, tag, n_random=24, with_zero=True):
    """Montgomery residues, `width` Fp coefficients per value (2, 6 or 12): 0, 1, -1, a single non-zero coefficient in each
    position, every coefficient p - 1, the upper half zero, non-canonical representatives (p for 0, x + p), random"""
    rnd = _rng("tower %d %s" % (width, tag))
    one = RP % P
    vals = []
    if with_zero:
        vals.append([0] * width)
    vals.append([one] + [0] * (width - 1))
    vals.append([P - one] + [0] * (width - 1))
    for k in range(width):
        for x in (one, P - 1, rnd.randrange(P)):
            v = [0] * width
            v[k] = x
            vals.append(v)
    vals.append([P - 1] * width)
    if width == 12:
        vals.append(_rand_flat(rnd, 6, P) + [0] * 6)                      # c1 = 0: the norm path of f12_inv
        vals.append([0] * 6 + _rand_flat(rnd, 6, P))
    vals.append([one] + [P] * (width - 1))                                # 1 with every zero written as p
    vals.append([one + P] + [P if k % 2 else 0 for k in range(1, width)])
    c = _rand_flat(rnd, width, P)
    vals.append([x + P for x in c])                                       # x + p throughout
    vals.append([x + P if k % 2 else x for k, x in enumerate(c)])
    vals.append([2 * P - 1] * width)
    vals += [_rand_flat(rnd, width) for _ in range(n_random)]
    return vals


_cyclotomic = {}


def cyclotomic_values(n=4):
    """Montgomery residues of n + 1 elements of the cyclotomic subgroup, 1 first: four by the easy part of the final
    exponentiation in the model, the rest products and conjugates of those (the subgroup is closed under both); from the
    second on, some coefficients in their non-canonical representative x + p (a different pattern for each element)"""
    if n not in _cyclotomic:
        rnd = _rng("cyclotomic")
        base = [f12_cyclotomic(shaped(F12_ONE, iter(_rand_flat(rnd, 12, P)))) for _ in range(4)]
        elems = list(base)
        while len(elems) < n:
            k = len(elems)
            x = f12_mul(elems[k - 1], base[k % 4])
            elems.append(f12_conj(x) if k % 3 == 0 else f12_mul(x, x) if k % 3 == 1 else x)
        out = [flat(mont(F12_ONE))]
        for i, x in enumerate(elems[:n]):
            m = flat(mont(x))
            out.append([v + P if (i and v < P and (i >> (k % 5)) & 1) else v for k, v in enumerate(m)])
        _cyclotomic[n] = out
    return _cyclotomic[n]


# --------------------------------------------------------------------------------------------- the hooks through ctypes
FORM_NAMES = {0: "fr", 1: "fp", 2: "fpl", 3: "fp2", 4: "fp2k3", 5: "fp2pair", 6: "tower", 7: "sqrt"}
CANON_OPS = {0: "fe_add", 1: "fe_sub", 2: "fe_neg", 3: "fe_dbl", 4: "fe_mul", 5: "fe_mul_b", 6: "fe_sqr", 7: "fe_to_mont",
             8: "fe_from_mont", 9: "fe_inv"}
LAZY_OPS = {0: "add", 1: "sub", 2: "neg", 3: "dbl", 4: "canon", 5: "is_zero", 6: "eq", 7: "mul", 8: "mul_tail", 9: "sqr",
            10: "mul2_sub", 11: "mul2_sub_tail", 12: "inv", 13: "fpl_add2", 14: "fpl_sub2"}
LANE_OPS = {0: "add", 1: "sub", 2: "neg", 3: "dbl", 4: "canon", 5: "is_zero", 6: "eq", 7: "mul", 9: "sqr", 13: "load_store",
            14: "one", 15: "curve_b"}
TOWER_OPS = {0: "f2_mul_xi", 1: "f2_mul_fp", 2: "f2_conj", 3: "f2_mul_small_3", 4: "f2_mul_small_4", 5: "f2_mul_small_12",
             6: "f6_mul", 7: "f6_mul_01", 8: "f6_mul_1", 9: "f6_mul_v", 10: "f6_inv", 11: "f12_mul", 12: "f12_sqr",
             13: "f12_mul_line", 14: "f12_inv", 15: "f12_conj", 16: "f12_frob1", 17: "f12_frob2", 18: "f12_cyc_sqr",
             19: "f12_cyc_exp_x", 20: "f12_is_one", 21: "f12_final_exp"}
SQRT_OPS = {0: "fp_sqrt", 1: "fp2_sqrt", 2: "fpl_half", 3: "fp_lex_largest", 4: "fp2_lex_largest"}


# the number of elements of every case: a filter that crept into a table builder shows here
TABLE_SIZES = {
    "fr-fe_add": 14595, "fr-fe_sub": 14595, "fr-fe_neg": 4101, "fr-fe_dbl": 4101, "fr-fe_mul": 15201, "fr-fe_mul_b": 15201,
    "fr-fe_sqr": 4101, "fr-fe_to_mont": 4101, "fr-fe_from_mont": 4101, "fr-fe_inv": 400,
    "fp-fe_add": 26787, "fp-fe_sub": 26787, "fp-fe_neg": 4149, "fp-fe_mul": 26787, "fp-fe_sqr": 4149,
    "fpl-add": 28302, "fpl-sub": 28302, "fpl-neg": 4153, "fpl-dbl": 4153, "fpl-canon": 4153, "fpl-is_zero": 4153, "fpl-eq": 28302,
    "fpl-mul": 34444, "fpl-mul_tail": 34444, "fpl-sqr": 4279, "fpl-mul2_sub": 9731, "fpl-mul2_sub_tail": 9731, "fpl-inv": 353,
    "fpl-fpl_add2": 28302, "fpl-fpl_sub2": 28302,
    "fp2-add": 82404, "fp2-sub": 82404, "fp2-neg": 25709, "fp2-dbl": 25709, "fp2-canon": 25709, "fp2-is_zero": 25709,
    "fp2-eq": 82404, "fp2-mul": 82404, "fp2-mul_tail": 82404, "fp2-sqr": 25709, "fp2-mul2_sub": 3411, "fp2-mul2_sub_tail": 3411,
    "fp2-inv": 335,
    "fp2k3-add": 18598, "fp2k3-sub": 18598, "fp2k3-neg": 36033, "fp2k3-dbl": 36033, "fp2k3-canon": 36033,
    "fp2k3-is_zero": 36033, "fp2k3-eq": 18598, "fp2k3-mul": 18598, "fp2k3-sqr": 36033, "fp2k3-load_store": 36033,
    "fp2k3-one": 821, "fp2k3-curve_b": 821,
    "fp2pair-add": 18598, "fp2pair-sub": 18598, "fp2pair-neg": 36033, "fp2pair-dbl": 36033, "fp2pair-canon": 36033,
    "fp2pair-is_zero": 36033, "fp2pair-eq": 18598, "fp2pair-mul": 18598, "fp2pair-sqr": 36033, "fp2pair-load_store": 36033,
    "fp2pair-one": 821, "fp2pair-curve_b": 821,
    "tower-f2_mul_xi": 24209, "tower-f2_mul_fp": 24209, "tower-f2_conj": 24209, "tower-f2_mul_small_3": 24209,
    "tower-f2_mul_small_4": 24209, "tower-f2_mul_small_12": 24209, "tower-f6_mul": 918, "tower-f6_mul_01": 357,
    "tower-f6_mul_1": 357, "tower-f6_mul_v": 51, "tower-f6_inv": 50, "tower-f12_mul": 1775, "tower-f12_sqr": 71,
    "tower-f12_mul_line": 825, "tower-f12_inv": 70, "tower-f12_conj": 71, "tower-f12_frob1": 71, "tower-f12_frob2": 71,
    "tower-f12_cyc_sqr": 41, "tower-f12_cyc_exp_x": 5, "tower-f12_is_one": 87, "tower-f12_final_exp": 8,
    "sqrt-fp_sqrt": 308, "sqrt-fp2_sqrt": 361, "sqrt-fpl_half": 4153, "sqrt-fp_lex_largest": 4157, "sqrt-fp2_lex_largest": 789,
}


def cases():
    """every (form, op) both tests run, with a readable id"""
    out = [(0, op) for op in CANON_OPS] + [(1, op) for op in (0, 1, 2, 4, 6)]
    out += [(2, op) for op in LAZY_OPS] + [(3, op) for op in LAZY_OPS if op < 13]
    out += [(f, op) for f in (4, 5) for op in LANE_OPS] + [(6, op) for op in TOWER_OPS] + [(7, op) for op in SQRT_OPS]
    return out


def case_id(case):
    form, op = case
    names = CANON_OPS if form < 2 else LAZY_OPS if form < 4 else LANE_OPS if form < 6 else TOWER_OPS if form == 6 else SQRT_OPS
    return "%s-%s" % (FORM_NAMES[form], names[op])


def shape(lib, form, op):
    out = (ctypes.c_size_t * 4)()
    assert lib.bh_test_field_ops_shape(form, op, out) == 0, (form, op)
    return tuple(int(x) for x in out)     # result bytes per element, flags per element, operand slot bytes, operands used


def pack(elems, slot, word=48):
    """values (nested Fp / Fr integers) -> an (n, slot) byte array, each integer `word` bytes little-endian, zero padded"""
    pad = bytes(slot)
    rows = []
    for e in elems:
        b = b"".join(v.to_bytes(word, "little") for v in flat(e))
        rows.append(b + pad[len(b):])
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(elems), slot).copy()


def unpack(rows, word=48):
    """an (n, k * word) byte array -> n lists of k integers"""
    out = []
    for row in rows:
        b = row.tobytes()
        out.append([int.from_bytes(b[i:i + word], "little") for i in range(0, len(b), word)])
    return out


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def operand_arrays(lib, form, op, operands):
    """operands: a list of tuples (one value per operand used) or of single values for a unary operation"""
    rbytes, nflags, slot, arity = shape(lib, form, op)
    word = 32 if form == 0 else 48
    cols = [[e] for e in operands] if arity == 1 else operands
    assert all(len(c) == arity for c in cols), (form, op, arity)
    arrs = [pack([c[k] for c in cols], slot, word) for k in range(arity)] + [None] * (4 - arity)
    return rbytes, nflags, arrs


def run_host(lib, form, op, operands):
    rbytes, nflags, arrs = operand_arrays(lib, form, op, operands)
    n = len(operands)
    raw = np.zeros((n, rbytes), dtype=np.uint8)
    flags = np.full((n, nflags), 0xFFFFFFFF, dtype=np.uint32)
    assert lib.bh_test_field_ops_host(form, op, _ptr(raw), _ptr(flags), *[_ptr(a) for a in arrs], n) == 0
    return raw, flags


def run_dev(lib, worker, form, op, operands):
    """the same through bh_test_field_ops_dev; the lane forms return (lane values, stored Fp2 values) as `raw`"""
    rbytes, nflags, arrs = operand_arrays(lib, form, op, operands)
    n = len(operands)
    bufs = []
    try:
        dev = []
        for a in arrs:
            if a is None:
                dev.append(None)
                continue
            d = worker.alloc(max(a.nbytes, 16))
            bufs.append(d)
            worker.upload(d, a)
            dev.append(d)
        raw = np.zeros(n * rbytes, dtype=np.uint8)
        flags = np.full((n, nflags), 0xFFFFFFFF, dtype=np.uint32)
        dr, df = worker.alloc(max(raw.nbytes, 16)), worker.alloc(max(flags.nbytes, 16))
        bufs += [dr, df]
        worker.upload(dr, raw)
        worker.upload(df, flags)
        assert lib.bh_test_field_ops_dev(worker.ctx, form, op, dr, df, *dev, n) == 0
        worker.download(raw, dr)
        worker.download(flags, df)
    finally:
        for d in bufs:
            worker.free(d)
    if form in (4, 5):
        lanes = nflags
        return (raw[:n * lanes * 48].reshape(n, lanes * 48), raw[n * lanes * 48:].reshape(n, 96)), flags
    return raw.reshape(n, rbytes), flags


# ------------------------------------------------------------------------------------------ operands of every case
_tables = {}


def operands_for(case):
    """the operand table of one (form, op): built once, shared by the host and the device run"""
    if case not in _tables:
        _tables[case] = _build_operands(*case)
    return _tables[case]


def _as2(flat12):
    return shaped(F2_ZERO, iter(flat12))


def _build_operands(form, op):
    if form in (0, 1):
        m, rbits, corners, wide = (Q, 256, FR_CANON, FR_WIDE) if form == 0 else (P, 384, FP_CANON, FP_WIDE[:0])
        tag = FORM_NAMES[form]
        if op in (0, 1):
            return binary_table(corners, m, m, tag)
        if op in (4, 5):
            # the canonical product is exact for a wide first operand too: a b / R + m < 2 m for b < m
            return binary_table(corners, m, m, tag) + [(w, c) for w in wide for c in corners]
        if op == 9:
            return unary_table([c for c in corners if c], m, tag, 300)
        return unary_table(corners, m, tag)
    if form == 2:
        if op in (0, 1, 6):
            return binary_table(FP_LAZY, P, 2 * P, "fpl")
        if op in (7, 8):
            return product_table("fpl")
        if op == 9:
            return unary_table(FP_LAZY + [w for w in FP_WIDE if w < (1 << 383)] + HIGH_LAZY + high_limb_values(1 << 383, 60, "sqr"),
                               2 * P, "fpl")
        if op in (10, 11):
            return fp_quad_table()
        if op in (13, 14):
            t = binary_table(FP_LAZY, P, 2 * P, "fpl")
            return [t[i] + t[(i * 13 + 5) % len(t)] for i in range(len(t))]
        if op == 12:
            return unary_table(FP_LAZY, 2 * P, "fpl", 200)
        return unary_table(FP_LAZY, 2 * P, "fpl")
    if form == 3:
        if op in (0, 1, 6, 7, 8):
            return fp2_binary_table()
        if op in (10, 11):
            return fp2_quad_table()
        if op == 12:
            return FP2_CORE + fp2_unary_table(100)[-100:]
        return fp2_unary_table()
    if form in (4, 5):
        tag = "%d" % op
        if op in (0, 1, 6, 7):
            core = [(a, b) for a in FP2_CORE[::3] for b in FP2_CORE[::5]]
            core += [(a, ((a[0] + P) % (2 * P), a[1])) for a in FP2_CORE] + [(a, a) for a in FP2_CORE]
            full = fp2_unary_table(0)
            core += [(a, full[(i * 37 + 11) % len(full)]) for i, a in enumerate(full[::3])]
            return lane_layout(core, tag, 2)
        if op in (14, 15):
            return lane_layout(FP2_CORE, tag, 1)
        return lane_layout(fp2_unary_table(0), tag, 1)
    if form == 6:
        return _tower_operands(op)
    return _sqrt_operands(op)


def _tower_operands(op):
    name = TOWER_OPS[op]
    width = 2 if name.startswith("f2_") else 6 if name.startswith("f6_") else 12
    as_val = {2: F2_ZERO, 6: F6_ZERO, 12: F12_ZERO}[width]
    rnd = _rng("tower ops " + name)

    def vals(tag, **kw):
        return [shaped(as_val, iter(v)) for v in tower_values(width, tag, **kw)]

    def f2s(tag, n):
        pool = [shaped(F2_ZERO, iter(v)) for v in tower_values(2, tag, n_random=8)]
        return [pool[(i * 7 + 3) % len(pool)] if i % 3 else _as2(_rand_flat(rnd, 2)) for i in range(n)]

    if name in ("f2_mul_xi", "f2_conj") or name.startswith("f2_mul_small"):
        return fp2_unary_table(500)
    if name == "f2_mul_fp":
        t = fp2_unary_table(500)
        return [(a, FP_LAZY[(i * 29 + 1) % len(FP_LAZY)] if i % 4 else rnd.randrange(2 * P)) for i, a in enumerate(t)]
    if name in ("f6_mul", "f12_mul"):
        a = vals("a")
        b = vals("b")
        return [(x, y) for x in a for y in b[::3]] + [(x, x) for x in a]
    if name == "f6_mul_01":
        a = vals("a")
        return [(x, y, z) for x in a for y, z in zip(f2s("x0", 7), f2s("x1", 7))]
    if name == "f6_mul_1":
        a = vals("a")
        return [(x, y) for x in a for y in f2s("y", 7)]
    if name == "f12_mul_line":
        a = vals("f", n_random=8)
        zero = F2_ZERO
        lines = list(zip(f2s("l0", 9), f2s("l2", 9), f2s("l3", 9)))
        l0, l2, l3 = lines[0]
        lines += [(zero, l2, l3), (l0, zero, l3), (l0, l2, zero), (zero, zero, l3), (zero, zero, zero), ((P, P), l2, (0, P))]
        return [(x,) + ln for x in a for ln in lines]
    if name in ("f6_inv", "f12_inv"):
        return vals("inv", with_zero=False)
    if name == "f12_cyc_sqr":
        return [shaped(F12_ZERO, iter(v)) for v in cyclotomic_values(40)]
    if name == "f12_cyc_exp_x":
        return [shaped(F12_ZERO, iter(v)) for v in cyclotomic_values()]
    if name == "f12_final_exp":
        pool = tower_values(12, "final exp", n_random=2, with_zero=False)
        # 1, -1, one single-coefficient element, all p - 1, c1 = 0, a non-canonical representative, two random values
        pick = [pool[0], pool[1], pool[2 + 3 * 7], pool[2 + 36], pool[2 + 37], pool[2 + 41], pool[-2], pool[-1]]
        return [shaped(F12_ZERO, iter(v)) for v in pick]
    if name == "f12_is_one":
        one = RP % P
        ones = [[one] + [0] * 11, [one + P] + [0] * 11, [one] + [P] * 11, [one + P] + [P, 0] * 5 + [P]]
        near = []
        for k in range(12):
            v = [one] + [0] * 11
            v[k] = (v[k] + 1) % (2 * P)
            near.append(v)
        return [shaped(F12_ZERO, iter(v)) for v in ones + near] + vals("is one")
    return vals("unary")     # f6_mul_v, f12_sqr, f12_conj, f12_frob1, f12_frob2


def _sqrt_operands(op):
    rnd = _rng("sqrt %d" % op)
    name = SQRT_OPS[op]
    if name == "fp_sqrt":
        vals = unary_table(FP_LAZY, 2 * P, "sqrt", 150)
        vals += [x * x % P * RP % P for x in (2, 3, P - 1, rnd.randrange(P), rnd.randrange(P))]
        return [(v, 0) for v in vals]
    if name == "fpl_half":
        return [(v, 0) for v in unary_table(FP_LAZY, 2 * P, "half")]
    if name == "fp_lex_largest":
        half = (P - 1) // 2
        edge = [mont(v) for v in (0, 1, half - 1, half, half + 1, half + 2, P - 1, P - 2)]
        return [(v, 0) for v in unary_table(FP_CANON + edge, P, "lex")]
    if name == "fp2_lex_largest":
        half = (P - 1) // 2
        edge = [mont(v) for v in (0, 1, half, half + 1, P - 1)]
        return [(a, b) for a in edge + FP_CANON[:12] for b in edge + FP_CANON[:12]] + [(rnd.randrange(P), rnd.randrange(P)) for _ in range(500)]
    # fp2_sqrt: pairs of the short corner list (c1 = 0 and c1 = p, the real path, among them), squares, random values
    vals = list(FP2_CORE)
    for _ in range(40):
        x = (rnd.randrange(P), rnd.randrange(P))
        vals.append(mont(f2_mul(x, x)))
    vals += [mont((x * x % P, 0)) for x in (2, 5, rnd.randrange(P))] + [mont((P - x * x % P, 0)) for x in (2, 5, rnd.randrange(P))]
    vals += [(rnd.randrange(2 * P), rnd.randrange(2 * P)) for _ in range(80)]
    return vals


# --------------------------------------------------------------------------------------------------------- expectations
def _lazy_ok(r, want_real=None, bound=None):
    """every coefficient below the bound (2p unless given), and the value congruent to the model's"""
    b = 2 * P if bound is None else bound
    if not all(0 <= v < b for v in flat(r)):
        return False
    return want_real is None or real(r) == fmap(lambda v: v % P, want_real)


def check(form, op, operands, raw, flags):
    """assert what `raw` / `flags` of one (form, op) must be; returns the number of elements checked"""
    n = len(operands)
    assert len(flags) == n
    if form in (0, 1):
        return _check_canon(form, op, operands, unpack(raw, 32 if form == 0 else 48), flags)
    if form == 2:
        return _check_fpl(op, operands, unpack(raw), flags)
    if form == 3:
        return _check_fp2(op, operands, unpack(raw), flags)
    if form in (4, 5):
        return _check_lanes(form, op, operands, raw, flags)
    if form == 6:
        return _check_tower(op, operands, unpack(raw), flags)
    return _check_sqrt(op, operands, unpack(raw), flags)


def _check_canon(form, op, operands, res, flags):
    m, r, rinv = (Q, RQ, RQ_INV) if form == 0 else (P, RP, RP_INV)
    for i, e in enumerate(operands):
        a, b = e if isinstance(e, tuple) else (e, 0)
        want = {0: (a + b) % m, 1: (a - b) % m, 2: -a % m, 3: 2 * a % m, 4: a * b * rinv % m, 5: a * b * rinv % m, 6: a * a * rinv % m,
                7: a * r % m, 8: a * rinv % m}.get(op)
        if op == 9:
            want = pow(a, m - 2, m) * r * r % m
        assert res[i] == [want], (case_id((form, op)), i, hex(a), hex(b))
    assert not flags.any()
    return len(operands)


def _check_fpl(op, operands, res, flags):
    name = LAZY_OPS[op]
    for i, e in enumerate(operands):
        t = e if isinstance(e, tuple) else (e,)
        a = t[0]
        r = res[i][0]
        ctx = (case_id((2, op)), i, [hex(v) for v in t], hex(r))
        f = int(flags[i][0])
        if name in ("add", "sub", "dbl", "neg"):
            want = {"add": a + (t[1] if len(t) > 1 else 0), "sub": a - (t[1] if len(t) > 1 else 0), "dbl": 2 * a, "neg": -a}[name]
            assert r < 2 * P and (r - want) % P == 0, ctx
            assert name != "neg" or a != 0 or r == 0, ctx          # -0 = 0, not 2p
        elif name == "canon":
            assert r == a % P, ctx
        elif name == "is_zero":
            assert f == (1 if a % P == 0 else 0) and r == a, ctx
        elif name == "eq":
            assert f == (1 if (a - t[1]) % P == 0 else 0) and r == a, ctx
        elif name in ("mul", "mul_tail"):
            assert (r * RP - a * t[1]) % P == 0 and r < a * t[1] // RP + P + 1, ctx
        elif name == "sqr":
            assert (r * RP - a * a) % P == 0 and r < a * a // RP + P + 1, ctx
        elif name in ("mul2_sub", "mul2_sub_tail"):
            b, c, d = t[1:]
            assert (r * RP - (a * b - c * d)) % P == 0 and r < (a * b + (2 * P - c) * d) // RP + P + 1, ctx
        elif name == "inv":
            assert r < 2 * P and r % P == pow(a, P - 2, P) * RP * RP % P, ctx
        else:
            b, c, d = t[1:]
            r1 = res[i][1]
            w0, w1 = (a + b, c + d) if name == "fpl_add2" else (a - b, c - d)
            assert r < 2 * P and r1 < 2 * P and (r - w0) % P == 0 and (r1 - w1) % P == 0, ctx
        if name not in ("is_zero", "eq"):
            assert f == 0, ctx
    return len(operands)


def _f2_expect(name, t):
    a = real(t[0])
    if name == "add":
        return f2_add(a, real(t[1]))
    if name == "sub":
        return f2_sub(a, real(t[1]))
    if name == "neg":
        return f2_neg(a)
    if name == "dbl":
        return f2_add(a, a)
    if name in ("mul", "mul_tail"):
        return f2_mul(a, real(t[1]))
    if name == "sqr":
        return f2_mul(a, a)
    if name in ("mul2_sub", "mul2_sub_tail"):
        return f2_sub(f2_mul(a, real(t[1])), f2_mul(real(t[2]), real(t[3])))
    if name == "inv":
        return f2_inv(a)
    if name in ("canon", "is_zero", "eq", "load_store"):
        return a
    if name == "one":
        return F2_ONE
    if name == "curve_b":
        return (4, 4)
    raise KeyError(name)


def _check_fp2(op, operands, res, flags):
    name = LAZY_OPS[op]
    for i, e in enumerate(operands):
        t = e if isinstance(e[0], tuple) else (e,)
        r = tuple(res[i])
        ctx = (case_id((3, op)), i, [[hex(v) for v in x] for x in t], [hex(v) for v in r])
        f = int(flags[i][0])
        assert _lazy_ok(r, _f2_expect(name, t)), ctx
        if name == "canon":
            assert r == (t[0][0] % P, t[0][1] % P), ctx
        if name == "neg":
            assert all(x != 0 or y == 0 for x, y in zip(t[0], r)), ctx
        want_flag = 0
        if name == "is_zero":
            want_flag = 1 if real(t[0]) == F2_ZERO else 0
        if name == "eq":
            want_flag = 1 if real(t[0]) == real(t[1]) else 0
        if name in ("is_zero", "eq"):
            assert r == tuple(t[0]), ctx
        assert f == want_flag, ctx
    return len(operands)


def _ladd(a, b):
    """fpl_add on integers: the representative in [0, 2p) it returns"""
    return a + b - 2 * P if a + b >= 2 * P else a + b


def _lsub(a, b):
    return a - b + 2 * P if a < b else a - b


def _check_lanes(form, op, operands, raw, flags):
    lanes = 3 if form == 4 else 2
    name = LANE_OPS[op]
    lane_vals, stored = unpack(raw[0]), unpack(raw[1])
    for i, e in enumerate(operands):
        t = e if isinstance(e[0], tuple) else (e,)
        lv, sv = lane_vals[i], stored[i]
        ctx = (case_id((form, op)), i, "lane position %d" % (i % (21 if form == 4 else 32)), [[hex(v) for v in x] for x in t],
               [hex(v) for v in lv])
        assert len(lv) == lanes and sv == lv[:2], ctx                      # F::store writes what the c0 and c1 lanes hold
        assert _lazy_ok(tuple(lv[:2]), _f2_expect(name, t)), ctx
        if lanes == 3:                                                     # the sum lane carries c0 + c1
            assert lv[2] < 2 * P and (lv[2] - lv[0] - lv[1]) % P == 0, ctx
        if lanes == 2 and name in ("mul", "sqr"):
            # a lane of a pair holds ONE Montgomery product (fused for the even lane of mul): the multiplier's own bound
            a0, a1 = t[0]
            if name == "mul":
                b0, b1 = t[1]
                sums = (a0 * b0 + a1 * (2 * P - b1), a0 * b1 + a1 * b0)
            else:
                sums = (_ladd(a1, a0) * _lsub(a0, a1), _ladd(a0, a0) * a1)
            assert lv[0] < sums[0] // RP + P + 1 and lv[1] < sums[1] // RP + P + 1, ctx
        if name == "canon":
            assert all(v < P for v in lv), ctx
        if name == "load_store":
            assert tuple(sv) == tuple(t[0]), ctx
        if name == "neg":
            assert all(x != 0 or y == 0 for x, y in zip(t[0], lv)), ctx
        if name == "one":
            assert lv[:2] == [RP % P, 0], ctx
        want_flag = 0
        if name == "is_zero":
            want_flag = 1 if real(t[0]) == F2_ZERO else 0
        if name == "eq":
            want_flag = 1 if real(t[0]) == real(t[1]) else 0
        assert [int(x) for x in flags[i]] == [want_flag] * lanes, ctx       # the same answer in every lane of the group
    return len(operands)


def _f6(x):
    return (x[0], x[1], F2_ZERO) if len(x) == 2 else x


def _tower_expect(name, t):
    a = real(t[0])
    if name == "f2_mul_xi":
        return f2_mul(a, XI)
    if name == "f2_mul_fp":
        return f2_scale(a, real(t[1]))
    if name == "f2_conj":
        return f2_conj(a)
    if name.startswith("f2_mul_small"):
        return f2_scale(a, int(name.rsplit("_", 1)[1]))
    if name == "f6_mul":
        return f6_mul(a, real(t[1]))
    if name == "f6_mul_01":
        return f6_mul(a, (real(t[1]), real(t[2]), F2_ZERO))
    if name == "f6_mul_1":
        return f6_mul(a, (F2_ZERO, real(t[1]), F2_ZERO))
    if name == "f6_mul_v":
        return f6_mul_v(a)
    if name == "f6_inv":
        return f6_inv(a)
    if name == "f12_mul":
        return f12_mul(a, real(t[1]))
    if name in ("f12_sqr", "f12_cyc_sqr"):
        return f12_mul(a, a)
    if name == "f12_mul_line":      # f ((l0 + l2 v) + (l3 v) w)
        return f12_mul(a, ((real(t[1]), real(t[2]), F2_ZERO), (F2_ZERO, real(t[3]), F2_ZERO)))
    if name == "f12_inv":
        return f12_inv(a)
    if name == "f12_conj":
        return f12_conj(a)
    if name == "f12_frob1":
        return f12_frob(a, 1)
    if name == "f12_frob2":
        return f12_frob(a, 2)
    if name == "f12_cyc_exp_x":     # x < 0, and the inverse of a cyclotomic element is its conjugate
        return f12_conj(f12_pow(a, X_ABS))
    if name == "f12_final_exp":
        return f12_pow(a, FINAL_EXP)
    if name == "f12_is_one":
        return a
    raise KeyError(name)


def _check_tower(op, operands, res, flags):
    name = TOWER_OPS[op]
    width = 2 if name.startswith("f2_") else 6 if name.startswith("f6_") else 12
    for i, e in enumerate(operands):
        t = e if name in ("f2_mul_fp", "f6_mul", "f6_mul_01", "f6_mul_1", "f12_mul", "f12_mul_line") else (e,)
        want = _tower_expect(name, t)
        r = shaped(want, iter(res[i][:width]))
        ctx = (case_id((6, op)), i, [hex(v) for v in flat(t)], [hex(v) for v in res[i][:width]])
        assert _lazy_ok(r, want, P if name == "f12_final_exp" else None), ctx
        want_flag = 0
        if name == "f12_is_one":
            want_flag = 1 if want == F12_ONE else 0
            assert flat(r) == flat(t[0]), ctx
        if name == "f12_final_exp":
            want_flag = 1 if want == F12_ONE else 0
        assert int(flags[i][0]) == want_flag, ctx
    return len(operands)


def _check_sqrt(op, operands, res, flags):
    name = SQRT_OPS[op]
    half = (P - 1) // 2
    for i, a in enumerate(operands):
        r, f = res[i], int(flags[i][0])
        ctx = (case_id((7, op)), i, [hex(v) for v in a], [hex(v) for v in r], f)
        if name == "fp_sqrt":
            x = real(a[0])
            assert f == (1 if fp_is_square(x) else 0), ctx                   # the Euler criterion
            assert r[0] < 2 * P, ctx
            assert real(r[0]) ** 2 % P == (x if f else -x % P), ctx          # a non-residue gives a root of -a
        elif name == "fp2_sqrt":
            x = real(a)
            assert f == (1 if f2_is_square(x) else 0), ctx                   # the norm test
            assert all(v < 2 * P for v in r), ctx
            if f:
                rr = real(tuple(r))
                assert f2_mul(rr, rr) == x, ctx
        elif name == "fpl_half":
            assert r[0] < 2 * P and (2 * r[0] - a[0]) % P == 0 and r[0] < 3 * P // 2 + 1, ctx
        elif name == "fp_lex_largest":
            assert f == (1 if real(a[0]) > half else 0), ctx
        else:
            x = real(a)
            assert f == (1 if (x[1] if a[1] != 0 else x[0]) > half else 0), ctx
        if name in ("fpl_half",):
            assert f == 0, ctx
    return len(operands)
