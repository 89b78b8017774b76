"""The stages of the Groth16 verifier (csrc/pairing_kernels.cuh) on Python integers, the operand tables the stage tests
share, and the record coding of the hooks bh_test_pairing_* (tests/test_pairing_stage_model_cpu.py pins the model and the
tables, tests/test_gpu_pairing_stages.py runs every kernel against it).

g2_dbl_step, g2_add_step, f12_mul_line_at and miller_loop_lines of csrc/fp12.cuh have no branches: the restatement below
predicts every line coefficient and every Fp12 coefficient of the raw Miller value exactly mod p, for any operands, on the
curve or off it.  Fields and the tower come from tests/field_model.py, the affine group law from tests/group_model.py.

Values: a G1 point (x, y), a G2 point ((x0, x1), (y0, y1)), the identity None; a line (l0, l2, l3) of Fp2 values; an Fp12
value ((a, b, c), (a, b, c)) in the memory order of fp12_t."""

import functools
import random

import numpy as np

from tests import field_model as fm
from tests import group_model as gm

P, Q = fm.P, fm.Q
RQ = fm.RQ
X_ABS = fm.X_ABS
MILLER_LINES = 68
PF_IDENTITY, PF_OFF_CURVE = 1, 2
PT_IS_INF = 16
PT_INVALID_BITS = (1, 2, 4, 8, 32, 64, 128)
PT_INVALID_MASK = sum(PT_INVALID_BITS)
OK, INVALID_POINT, POINT_AT_INFINITY, INVALID_PROOF = 0, 6, 7, 9
COLSUM_THREADS, COLSUM_BLOCKS = 256, 64
SENTINEL = 0xA5
CANONICAL, MONT = 0, 1          # BH_SCALARS_CANONICAL / BH_SCALARS_MONT
WIDTHS = (8, 4, 2, 1)


# ----------------------------------------------------------------------------------------------- lines and the Miller loop
def _small(a, k):
    return fm.f2_scale(a, k)


def g2_dbl_step(t):
    """T <- 2T; line = (Y^2 - 3b'Z^2, -3X^2, 2YZ) with b' = 4 xi"""
    x, y, z = t
    a = fm.f2_mul(x, y)
    b = fm.f2_mul(y, y)
    c = fm.f2_mul(z, z)
    e = _small(fm.f2_mul(c, fm.XI), 12)
    f = _small(e, 3)
    h = fm.f2_sub(fm.f2_sub(fm.f2_mul(fm.f2_add(y, z), fm.f2_add(y, z)), b), c)
    xx = fm.f2_mul(x, x)
    line = (fm.f2_sub(b, e), fm.f2_neg(_small(xx, 3)), h)
    x3 = fm.f2_mul(fm.f2_add(a, a), fm.f2_sub(b, f))
    s = fm.f2_add(b, f)
    y3 = fm.f2_sub(fm.f2_mul(s, s), _small(fm.f2_mul(e, e), 12))
    z3 = fm.f2_mul(_small(b, 4), h)
    return (x3, y3, z3), line


def g2_add_step(t, q):
    """T <- T + Q (Q affine); line = (th xQ - la yQ, -th, la)"""
    x, y, z = t
    xq, yq = q
    th = fm.f2_sub(y, fm.f2_mul(yq, z))
    la = fm.f2_sub(x, fm.f2_mul(xq, z))
    line = (fm.f2_sub(fm.f2_mul(th, xq), fm.f2_mul(la, yq)), fm.f2_neg(th), la)
    c = fm.f2_mul(th, th)
    d = fm.f2_mul(la, la)
    e = fm.f2_mul(la, d)
    f = fm.f2_mul(z, c)
    g = fm.f2_mul(x, d)
    h = fm.f2_sub(fm.f2_sub(fm.f2_add(e, f), g), g)
    x3 = fm.f2_mul(la, h)
    y3 = fm.f2_sub(fm.f2_mul(th, fm.f2_sub(g, h)), fm.f2_mul(e, y))
    return (x3, y3, fm.f2_mul(z, e)), line


@functools.lru_cache(maxsize=None)
def g2_lines(q):
    """the 68 lines of the affine point q (not the identity) in loop order"""
    t = (q[0], q[1], fm.F2_ONE)
    out = []
    for i in range(62, -1, -1):
        t, l = g2_dbl_step(t)
        out.append(l)
        if (X_ABS >> i) & 1:
            t, l = g2_add_step(t, q)
            out.append(l)
    assert len(out) == MILLER_LINES
    return tuple(out)


def line_at(line, p):
    """l0 + (l2 xP) w^2 + (l3 yP) w^3 as an Fp12 value"""
    return ((line[0], fm.f2_scale(line[1], p[0]), fm.F2_ZERO), (fm.F2_ZERO, fm.f2_scale(line[2], p[1]), fm.F2_ZERO))


def f12_mul_line_at(f, line, p):
    return fm.f12_mul(f, line_at(line, p))


def miller_multi(pairs):
    """the product of f_{|x|,Q}(P) over (P, lines of Q) under one chain of squarings (miller3_kernel; one pair:
    miller_loop_lines)"""
    f = fm.F12_ONE
    k = 0
    for i in range(62, -1, -1):
        if i != 62:
            f = fm.f12_mul(f, f)
        for _ in range(2 if (X_ABS >> i) & 1 else 1):
            for p, lines in pairs:
                f = f12_mul_line_at(f, lines[k], p)
            k += 1
    return f


@functools.lru_cache(maxsize=None)
def miller_loop_lines(p, lines):
    return miller_multi([(p, lines)])


def miller(p, q):
    """what miller_kernel leaves for the pair: 1 when either side is the identity"""
    return fm.F12_ONE if p is None or q is None else miller_loop_lines(p, g2_lines(q))


def f12_product(values):
    r = fm.F12_ONE
    for v in values:
        r = fm.f12_mul(r, v)
    return r


# ------------------------------------------------------------------------------------------------------------- the groups
def on_curve(g, pt):
    return gm.on_curve(g, pt)


@functools.lru_cache(maxsize=None)
def g1_mul(pt, k):
    """[k] pt by double-and-add over the integer k as it is (k may exceed q; pt may lie off the subgroup or off the curve:
    the law of y^2 = x^3 + b does not read b)"""
    return gm.mul(1, pt, k)


def g1_sum(points):
    acc = None
    for pt in points:
        acc = gm.add(1, acc, pt)
    return acc


def scalar_int(raw, fmt):
    """the integer scalar_bits makes of a 32-byte scalar: a canonical value as it is, a Montgomery one decoded"""
    return raw * fm.RQ_INV % Q if fmt == MONT else raw


def scalar_raw(v, fmt):
    """the 32-byte word that names v: v itself (any v < 2^256), or its Montgomery form (v < q)"""
    if fmt == MONT:
        assert v < Q
        return v * RQ % Q
    return v


# ------------------------------------------------------------------------------------------------------------ column sums
def colsum_nb(n):
    return min(COLSUM_BLOCKS, (n + COLSUM_THREADS - 1) // COLSUM_THREADS)


def colsum(z, rows, ncol, acc0, fmt, nb):
    """z[j], rows[j][i] raw words -> (part[col][block], acc[col]) as integers mod q (not Montgomery)"""
    zs = [scalar_int(v, fmt) % Q for v in z]
    part = [[0] * nb for _ in range(ncol)]
    for col in range(ncol):
        for b in range(nb):
            s = 0
            for first in range(b * COLSUM_THREADS, len(z), nb * COLSUM_THREADS):
                for j in range(first, min(first + COLSUM_THREADS, len(z))):
                    s += zs[j] if col == 0 else zs[j] * scalar_int(rows[j][col - 1], fmt)
            part[col][b] = s % Q
    return part, [(acc0[col] + sum(part[col])) % Q for col in range(ncol)]


# ------------------------------------------------------------------------------------------------------- the window table
def table_shape(w):
    return 256 // w, (1 << w) - 1          # windows, entries per window


def table_bytes(n_in, w):
    windows, entries = table_shape(w)
    return n_in * windows * entries * 96


def ic_table(ic, w):
    """entry [i][win][d - 1] = [d 2^(w win)] ic[i]"""
    windows, entries = table_shape(w)
    out = []
    for pt in ic:
        rows = []
        base = pt
        for _ in range(windows):
            row, acc = [], None
            for _d in range(entries):
                acc = gm.add(1, acc, base)
                row.append(acc)
            rows.append(row)
            for _k in range(w):
                base = gm.dbl(1, base)
        out.append(rows)
    return out


def digits(k, w):
    windows, entries = table_shape(w)
    return [(k >> (w * win)) & entries for win in range(windows)]


def accumulate_terms(table, w, scalars):
    """the table entries ic_accumulate_kernel adds for one proof, in its order (identity entries and zero digits skipped)"""
    terms = []
    for i, k in enumerate(scalars):
        for win, d in enumerate(digits(k, w)):
            if d and table[i][win][d - 1] is not None:
                terms.append(table[i][win][d - 1])
    return terms


def ic_accumulate(ic0, ic, scalars):
    """acc_j = ic_0 + sum_i a_i ic_{i+1} by the affine law"""
    return g1_sum([g1_mul(pt, k) for pt, k in zip(ic, scalars) if pt is not None] + [ic0])


# ---------------------------------------------------------------------------------------------------------- the verdict
def status_error(word):
    """proof_status_error: the first bad element in the order a, b, c"""
    for k in range(3):
        s = (word >> (8 * k)) & 0xFF
        if s & PT_INVALID_MASK:
            return INVALID_POINT
        if s & PT_IS_INF:
            return POINT_AT_INFINITY
    return OK


def verdict(word, pflag, qflag, is_one):
    """word None: the proofs did not come as bytes"""
    v = OK if word is None else status_error(word)
    if v != OK:
        return v
    if (pflag | qflag) & PF_OFF_CURVE:
        return INVALID_POINT
    return OK if is_one == 1 else INVALID_PROOF


# --------------------------------------------------------------------------------------------------------- record coding
def fp_bytes(v):
    return int(v).to_bytes(48, "little")


def mont_bytes(x, lazy=0):
    """the Montgomery words of the Fp coefficients of x in memory order; coefficient k is written as v + p (still < 2p)
    where bit k % 64 of `lazy` is set"""
    return b"".join(fp_bytes(v + P if (lazy >> (k % 64)) & 1 else v) for k, v in enumerate(fm.flat(fm.mont(x))))


def g1_rec(pt):
    return b"\0" * 96 if pt is None else mont_bytes(pt)


def g2_rec(pt):
    return b"\0" * 192 if pt is None else mont_bytes(pt)


def proof_rec(a, b, c):
    return g1_rec(a) + g2_rec(b) + g1_rec(c)


def lines_rec(lines, lazy=0):
    return mont_bytes(lines, lazy)


def fr_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def words(raw, size):
    """little-endian integers of `size` bytes each"""
    raw = bytes(raw)
    assert len(raw) % size == 0
    return [int.from_bytes(raw[k:k + size], "little") for k in range(0, len(raw), size)]


def decode_lazy(raw, like, bound=2 * P):
    """raw Fp words -> the values with the nesting of `like`; every word must lie below `bound`"""
    vals = words(raw, 48)
    assert all(v < bound for v in vals), "an Fp coefficient is not below %s" % ("p" if bound == P else "2p")
    return fm.shaped(like, iter([v * fm.RP_INV % P for v in vals]))


def decode_g1(raw):
    """a canonical affine record -> the point; the identity is the all-zero record and nothing else"""
    raw = bytes(raw)
    if raw == b"\0" * 96:
        return None
    pt = decode_lazy(raw, (0, 0), bound=P)
    assert pt != (0, 0), "a non-zero record that reads as the identity"
    return pt


def is_sentinel(raw):
    return bytes(raw) == bytes([SENTINEL]) * len(raw)


# ---------------------------------------------------------------------------------------------------------- operand tables
def rng(tag):
    return random.Random("pairing stages " + tag)


@functools.lru_cache(maxsize=None)
def g1_off_subgroup():
    """a point of E(Fp) outside the subgroup of order q: the first x = 1, 2, ... with x^3 + 4 a square"""
    for x in range(1, 100):
        y = fm.fp_sqrt((x ** 3 + 4) % P)
        if y is not None and gm.mul(1, (x, y), Q) is not None:
            return (x, y)
    raise AssertionError


@functools.lru_cache(maxsize=None)
def g1_points():
    """class -> G1 points; every class the stage tests name"""
    rnd = rng("g1")
    gen = gm.GEN[1]
    return {
        "generator": [gen],
        "random": [gm.mul(1, gen, rnd.randrange(1, Q)) for _ in range(3)],
        "order3": [(0, 2), (0, P - 2)],
        "off_subgroup": [g1_off_subgroup()],
        "off_curve": [(P - 1, P - 1), (gen[0], (gen[1] + 1) % P)],
        "identity": [None],
    }


@functools.lru_cache(maxsize=None)
def g2_points():
    rnd = rng("g2")
    gen = gm.GEN[2]
    special = gm.special_points(2)
    return {
        "generator": [gen],
        "random": [gm.mul(2, gen, rnd.randrange(1, Q)) for _ in range(2)],
        "x_c1_zero": [pt for pt in special if pt[0][1] == 0 and pt[0][0] != 0][:1],
        "x_c0_zero": [pt for pt in special if pt[0][0] == 0 and pt[0][1] != 0][:1],
        "off_subgroup": [pt for pt in special if pt[0][1] == 0 and pt[0][0] != 0][1:2],
        "off_curve": [(gen[0], fm.f2_add(gen[1], fm.F2_ONE))],
        "identity": [None],
    }


def lane_plan(classes, n, hot=(0, 63, 64)):
    """n (class, point) picks: every class in turn from lane 0 on, and - one call per rotation r - class r at the lanes of
    `hot` that exist; returns a function of the rotation"""
    names = sorted(classes)

    def plan(rot):
        out = []
        for lane in range(n):
            name = names[(rot + (0 if lane in hot else lane)) % len(names)]
            pts = classes[name]
            out.append((name, pts[lane % len(pts)]))
        return out

    return plan, len(names)


Z_EDGES = (1, 2, Q - 1, Q + 1, (1 << 256) - 1)
FR_EDGES = (0, 1, Q - 1, Q, Q + 1, (1 << 256) - 1)


def z_values(fmt, n, tag):
    """z_j for proof_prep: the edge values (canonical: any 256-bit value; Montgomery: the forms of values < q), then
    seeded random ones; returns (integers as scalar_bits reads them, raw words)"""
    rnd = rng("z " + tag)
    vals = [v for v in Z_EDGES if fmt == CANONICAL or v < Q]
    vals = [vals[j] if j < len(vals) else rnd.randrange(1, Q if fmt == MONT else 1 << 256) for j in range(n)]
    return vals, [scalar_raw(v, fmt) for v in vals]


def random_f12_lazy(rnd):
    """raw words in [0, 2p) of one Fp12 value"""
    return [rnd.randrange(2 * P) for _ in range(12)]


def f12_of_raw(raw12):
    return fm.shaped(fm.F12_ONE, iter([v * fm.RP_INV % P for v in raw12]))


def to_u32(values):
    return np.array(list(values), dtype=np.uint32)


# -------------------------------------------------------------------------------------------- a key with known discrete logs
class ScalarKey:
    """A verifying key whose every element is a known multiple of the generators, so that valid proofs of any statement are
    made from scalars alone: e(A, B) = e(alpha, beta) e(acc, gamma) e(C, delta) with acc = ic_0 + sum x_i ic_i holds
    exactly when r s = a b + (c_0 + sum x_i c_i) g + c d for A = [r] G1, B = [s] G2, C = [c] G1."""

    def __init__(self, n_inputs, tag):
        rnd = rng("key " + tag)
        self.a, self.b, self.g, self.d = (rnd.randrange(1, Q) for _ in range(4))
        self.c = [rnd.randrange(1, Q) for _ in range(n_inputs + 1)]
        self.rnd = rnd
        g1, g2 = gm.GEN[1], gm.GEN[2]
        self.alpha = gm.mul(1, g1, self.a)
        self.beta, self.gamma, self.delta = (gm.mul(2, g2, k) for k in (self.b, self.g, self.d))
        self.ic = [gm.mul(1, g1, k) for k in self.c]

    def proof(self, inputs):
        """a valid proof (A, B, C) of the statement `inputs` (integers; read mod q)"""
        r, s = self.rnd.randrange(1, Q), self.rnd.randrange(1, Q)
        acc = (self.c[0] + sum(x * k for x, k in zip(inputs, self.c[1:]))) % Q
        c = (r * s - self.a * self.b - acc * self.g) * pow(self.d, -1, Q) % Q
        return gm.mul(1, gm.GEN[1], r), gm.mul(2, gm.GEN[2], s), gm.mul(1, gm.GEN[1], c)
