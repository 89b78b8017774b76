"""The group law of G1 and G2 on Python integers, raw XYZZ operand tables, and the expectations for every form x operation
of bh_test_group_ops_dev / _host (tests/test_group_model_cpu.py pins the model and runs the one-lane forms through the host
build, tests/test_gpu_group_law.py runs every form on the device).

A point (x, y) is REPRESENTED by the record (x l^2, y l^3, l^2, l^3) for any l != 0, every Fp coefficient a Montgomery
residue written either as its canonical value v or as v + p (both lie in [0, 2p), the domain of the lazily reduced
arithmetic of csrc/ff.cuh).  The kernels meet such records in every merge: two partial sums with unrelated l, whose
equality must be read off cross-multiplied coordinates whose difference comes out as 0 or as p.  The affine law here is
written over tests/field_model.py; test_group_model_cpu.py pins it against oracle/pyref and oracle/c."""

import ctypes
import random
from collections import namedtuple

import numpy as np

from oracle.pyref import bls12_381 as bls
from tests import field_model as fm

P = fm.P
ONE = fm.RP % P          # the Montgomery residue of 1


# ------------------------------------------------------------------------------------------------------- the affine law
class _Fp:
    width, zero, one, b = 1, 0, 1, bls.G1_B
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    neg = staticmethod(lambda a: -a % P)
    inv = staticmethod(lambda a: pow(a, -1, P))


class _Fp2:
    width, zero, one, b = 2, fm.F2_ZERO, fm.F2_ONE, bls.G2_B
    add, sub, mul, neg = staticmethod(fm.f2_add), staticmethod(fm.f2_sub), staticmethod(fm.f2_mul), staticmethod(fm.f2_neg)

    @staticmethod
    def inv(a):
        n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)       # raises on zero: nothing here inverts zero
        return (a[0] * n % P, -a[1] * n % P)


FIELDS = {1: _Fp, 2: _Fp2}
GEN = {1: bls.G1_GEN, 2: bls.G2_GEN}


def on_curve(g, pt):
    F = FIELDS[g]
    return pt is None or F.mul(pt[1], pt[1]) == F.add(F.mul(F.mul(pt[0], pt[0]), pt[0]), F.b)


def neg(g, pt):
    return None if pt is None else (pt[0], FIELDS[g].neg(pt[1]))


def dbl(g, pt):
    F = FIELDS[g]
    if pt is None or pt[1] == F.zero:
        return None
    x, y = pt
    xx = F.mul(x, x)
    lam = F.mul(F.add(F.add(xx, xx), xx), F.inv(F.add(y, y)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x), x)
    return (x3, F.sub(F.mul(lam, F.sub(x, x3)), y))


def add(g, p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    F = FIELDS[g]
    if p1[0] == p2[0]:
        return dbl(g, p1) if p1[1] == p2[1] else None
    lam = F.mul(F.sub(p2[1], p1[1]), F.inv(F.sub(p2[0], p1[0])))
    x3 = F.sub(F.sub(F.mul(lam, lam), p1[0]), p2[0])
    return (x3, F.sub(F.mul(lam, F.sub(p1[0], x3)), p1[1]))


def mul(g, pt, k):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = dbl(g, acc)
        if bit == "1":
            acc = add(g, acc, pt)
    return acc


def classify(g, p1, p2):
    """the branch an addition of two points takes, from the points alone"""
    if p1 is None or p2 is None:
        return "both_identity" if p1 is None and p2 is None else "a_identity" if p1 is None else "b_identity"
    if p1[0] != p2[0]:
        return "general"
    return "same" if p1[1] == p2[1] else "opposite"


# -------------------------------------------------------------------------------------------------------------- points
_pools = {}


def subgroup_points(g, n=256):
    """k * generator for k = 1 .. n"""
    pool = _pools.setdefault(g, [GEN[g]])
    while len(pool) < n:
        pool.append(add(g, pool[-1], GEN[g]))
    return pool[:n]


_specials = {}


def special_points(g):
    """G1: (0, 2) and (0, p - 2), of order 3, whose U1 = U2 = 0 in any representation.  G2: curve points found by trying
    small x until x^3 + 4 (1 + u) is a square - x.c1 = 0 and x.c0 = 0 - with both signs of y; they lie off the subgroup of
    order q, where the formulas hold just as well.  x = 0 is tried too and gives nothing: 4 (1 + u) has norm 32, and 2 is
    not a square mod p (p = 3 mod 8), so the twist has no point with x = 0 (test_group_model_cpu.py asserts it)"""
    if g not in _specials:
        if g == 1:
            _specials[g] = [(0, 2), (0, P - 2)]
        else:
            out = []
            for shape in ("x = 0", "x.c1 = 0", "x.c0 = 0"):
                for k in range(1, 200):
                    x = (0, 0) if shape == "x = 0" else (k, 0) if shape == "x.c1 = 0" else (0, k)
                    y = fm.f2_sqrt(fm.f2_add(fm.f2_mul(fm.f2_mul(x, x), x), _Fp2.b))
                    if y is not None:
                        out += [(x, y), (x, fm.f2_neg(y))]
                        break
                    if shape == "x = 0":
                        break
            _specials[g] = out
    return _specials[g]


def _rng(tag):
    return random.Random("group law " + tag)


def _point_source(g, tag):
    """an endless supply of non-identity points: subgroup points of either sign, every seventh a special point"""
    rnd = _rng("points " + tag)
    pool, special = subgroup_points(g), special_points(g)
    i = 0
    while True:
        i += 1
        if i % 7 == 0:
            yield special[(i // 7) % len(special)]
        else:
            pt = pool[rnd.randrange(len(pool))]
            yield neg(g, pt) if rnd.randrange(2) else pt


def _lambda_source(g, tag):
    """non-zero l: 1, 2, p - 1, (p +- 1) / 2, values whose Montgomery residue has every limb near its maximum, seeded random
    values; in Fp2 pairs of those, with c0 = 0 and c1 = 0 among them.  No value is handed out twice."""
    rnd = _rng("lambda " + tag)
    fixed = [1, 2, P - 1, (P - 1) // 2, (P + 1) // 2] + [h * fm.RP_INV % P for h in fm.high_limb_values(P, 24, "lambda " + tag)]
    seen = set()
    i = 0
    while True:
        i += 1

        def one():
            return fixed[rnd.randrange(len(fixed))] if rnd.randrange(3) == 0 else rnd.randrange(1, P)

        if g == 1:
            lam = fixed[i - 1] if i <= len(fixed) else rnd.randrange(1, P)
        elif i <= len(fixed):
            lam = (fixed[i - 1], 0) if i % 3 == 0 else (0, fixed[i - 1]) if i % 3 == 1 else (fixed[i - 1], fixed[-i])
        else:
            lam = (one(), one())
        if lam in seen:
            continue
        seen.add(lam)
        yield lam


def represent(g, pt, lam, mask):
    """the flat raw record (X, Y, ZZ, ZZZ) of pt scaled by lam; coefficient k is written as v + p where bit k of mask is set"""
    F = FIELDS[g]
    l2 = F.mul(lam, lam)
    l3 = F.mul(l2, lam)
    coeffs = fm.flat(fm.mont((F.mul(pt[0], l2), F.mul(pt[1], l3), l2, l3)))
    return tuple(v + P if (mask >> k) & 1 else v for k, v in enumerate(coeffs))


def affine_record(g, pt):
    """canonical Montgomery (x, y); the identity is the all-zero record"""
    return (0,) * (2 * FIELDS[g].width) if pt is None else tuple(fm.flat(fm.mont(pt)))


def identity_record(g, rnd=None):
    """rnd None: the all-zero record.  Otherwise an identity that carries non-zero X and Y, each coefficient of ZZ written
    as 0 or as p; ZZZ likewise, or - every other time - any non-zero value: ZZ alone says whether a record is the identity"""
    w = FIELDS[g].width
    if rnd is None:
        return (0,) * (4 * w)
    xy = [rnd.randrange(1, 2 * P) for _ in range(2 * w)]
    zz = [P * rnd.randrange(2) for _ in range(w)]
    zzz = [rnd.randrange(1, 2 * P) for _ in range(w)] if rnd.randrange(2) else [P * rnd.randrange(2) for _ in range(w)]
    return tuple(xy + zz + zzz)


def decode(g, rec, strict=True):
    """a raw XYZZ record -> None when ZZ = 0 mod p, else the affine point (x, y) = (X / ZZ, Y / ZZZ); a record with
    ZZ^3 != ZZZ^2 is refused (strict) or reported as the string "inconsistent" (not strict)"""
    F = FIELDS[g]
    w = F.width
    x, y, zz, zzz = (fm.real(rec[k * w] if w == 1 else tuple(rec[k * w:(k + 1) * w])) for k in range(4))
    if zz == F.zero:
        return None
    if F.mul(F.mul(zz, zz), zz) != F.mul(zzz, zzz):
        assert not strict, "ZZ^3 != ZZZ^2"
        return "inconsistent"
    return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


# -------------------------------------------------------------------------------------------------------------- tables
# cls: the branch class, from the model alone; a, b: flat operand records (None where the operation has none; for the trees
# a is the list of the group's records); want: the model's affine result (None = identity)
Case = namedtuple("Case", "cls a b want")

FORMS = {0: "g1", 1: "g1k2", 2: "g2", 3: "g2k3", 4: "g2pair", 5: "g2k6"}
GROUP = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 5: 2}
LANES = {0: 1, 1: 2, 2: 1, 3: 3, 4: 2, 5: 6}
ELEMENT_PER_WAVE = {0: 64, 1: 32, 2: 64, 3: 21, 4: 32, 5: 8}      # workers of a wavefront in the one-operation kernels
TREE_PER_WAVE = {0: 64, 1: 32, 2: 64, 3: 16, 4: 32, 5: 8}         # ... and in the trees (a power of two)
OPS = {0: "add", 1: "add_alias", 2: "madd", 3: "madd_prefetch", 4: "dbl", 5: "dbl_affine", 6: "from_affine", 7: "to_affine",
       8: "is_identity", 9: "load_store", 10: "tree", 11: "block_sum"}
OP = {v: k for k, v in OPS.items()}
B_XYZZ, B_AFFINE = ("add", "add_alias"), ("madd", "madd_prefetch", "dbl_affine", "from_affine")
NO_A = ("dbl_affine", "from_affine")
CLASSES = {
    "add": ("general", "same", "opposite", "a_identity", "b_identity", "both_identity", "dirty_identity"),
    "madd": ("general", "same", "opposite", "a_identity", "b_identity", "both_identity", "dirty_identity"),
    "dbl": ("general", "a_identity", "dirty_identity", "y_zero"),
    "dbl_affine": ("general",),
    "from_affine": ("general", "b_identity"),
    "to_affine": ("general", "a_identity", "dirty_identity"),
    "is_identity": ("general", "a_identity", "dirty_identity"),
    "load_store": ("general", "a_identity", "dirty_identity"),
}
CLASSES["add_alias"], CLASSES["madd_prefetch"] = CLASSES["add"], CLASSES["madd"]
ARRANGEMENTS = ("same_point", "alternating", "doubling_chain", "all_identity", "single", "distinct")
PER_CLASS_INTERLEAVED, PER_CLASS_RUN = 64, 128      # a run of 128 covers a whole wavefront wherever it starts
GROUPS_PER_ARRANGEMENT = 24                         # per tree width G
BLOCK_CASES_PER_ARRANGEMENT = 64


def form_ops(form):
    if form in (1, 5):
        return ("add", "add_alias", "load_store")
    return tuple(n for n in OPS.values() if n not in ("load_store", "tree", "block_sum") and (n != "to_affine" or form in (0, 2)))


def tree_widths(form):
    return [g for g in (2, 4, 8, 16, 32, 64) if g <= TREE_PER_WAVE[form]]


def cases():
    """every (form, op, G) the tests run; G = 0 except for the trees"""
    out = []
    for form in FORMS:
        out += [(form, OP[n], 0) for n in form_ops(form)]
        out += [(form, OP["tree"], g) for g in tree_widths(form)] + [(form, OP["block_sum"], 0)]
    return out


def case_id(case):
    form, op, G = case
    return "%s-%s%s" % (FORMS[form], OPS[op], "-G%d" % G if G else "")


def _builder(g, name):
    """a function class -> Case for one operation; every call draws fresh points, l values and representation masks"""
    rnd = _rng("%d %s" % (g, name))
    pts, lams = _point_source(g, name), _lambda_source(g, "%d %s" % (g, name))
    w = FIELDS[g].width
    base = {"add_alias": "add", "madd_prefetch": "madd"}.get(name, name)

    def mask_pair():
        m1 = rnd.randrange(1 << (4 * w))
        m2 = rnd.randrange(1 << (4 * w))
        return (m1, m2) if m1 != m2 else (m1, m1 ^ 1)

    def rep(pt, m):
        return represent(g, pt, next(lams), m)

    def general_pair():
        while True:
            p1, p2 = next(pts), next(pts)
            if p1[0] != p2[0]:
                return p1, p2

    def build(cls, k):
        m1, m2 = mask_pair()
        if base in ("add", "madd"):
            second = (lambda pt, m: rep(pt, m)) if base == "add" else (lambda pt, m: affine_record(g, pt))
            zero_b = identity_record(g) if base == "add" else affine_record(g, None)
            if cls == "general":
                p1, p2 = general_pair()
            elif cls in ("same", "opposite"):
                p1 = next(pts)
                p2 = p1 if cls == "same" else neg(g, p1)
            elif cls == "a_identity":
                p1, p2 = None, next(pts)
            elif cls == "b_identity":
                p1, p2 = next(pts), None
            elif cls == "both_identity":
                p1, p2 = None, None
            else:   # dirty_identity: identities that carry non-zero X, Y
                which = k % 3 if base == "add" else 2 * (k % 2)      # add: a / b / both; madd: a with a base / with none
                p1 = next(pts) if which == 1 else None
                p2 = next(pts) if which == 0 else None
                a = identity_record(g, rnd) if p1 is None else rep(p1, m1)
                b = second(p2, m2) if p2 is not None else identity_record(g, rnd) if base == "add" else zero_b
                return Case(cls, a, b, add(g, p1, p2))
            assert classify(g, p1, p2) == cls
            a = identity_record(g) if p1 is None else rep(p1, m1)
            b = zero_b if p2 is None else second(p2, m2)
            return Case(cls, a, b, add(g, p1, p2))
        if base in ("dbl_affine", "from_affine"):
            pt = next(pts) if cls == "general" else None
            return Case(cls, None, affine_record(g, pt), dbl(g, pt) if base == "dbl_affine" else pt)
        # one raw operand: dbl, to_affine, is_identity, load_store
        if cls == "general":
            pt = next(pts)
            a = rep(pt, m1)
        elif cls == "a_identity":
            pt, a = None, identity_record(g)
        elif cls == "dirty_identity":
            pt, a = None, identity_record(g, rnd)
        else:   # y_zero: a record no curve point has, the documented early exit of the doubling
            pt = None
            a = list(rep(next(pts), m1))
            a[w:2 * w] = [P * rnd.randrange(2) for _ in range(w)]
            a = tuple(a)
        return Case(cls, a, None, dbl(g, pt) if base == "dbl" else pt)

    return build


_tables = {}


def operands_for(case):
    """the table of one (form, op, G): built once per (group, op, G), shared by every form of the group and by the host
    and the device run"""
    form, op, G = case
    g, name = GROUP[form], OPS[op]
    key = (g, name, G if name == "tree" else 4 * TREE_PER_WAVE[form] if name == "block_sum" else 0)
    if key not in _tables:
        _tables[key] = _build_sums(g, key[2], name) if name in ("tree", "block_sum") else _build_elements(g, name)
    return _tables[key]


def _build_elements(g, name):
    """interleaved: 64 rounds of one case of every class, so that neighbouring workers of a wavefront take different
    branches; then a run of 128 cases of each class, which holds a whole wavefront of every form wherever it starts; then
    general cases (or the only class) until the length is no multiple of 8 or 21, so that the last wavefront is ragged"""
    classes = CLASSES[name]
    build = _builder(g, name)
    out = [build(c, k) for k in range(PER_CLASS_INTERLEAVED) for c in classes]
    for c in classes:
        out += [build(c, k) for k in range(PER_CLASS_RUN)]
    while len(out) % 8 == 0 or len(out) % 21 == 0:
        out.append(build(classes[0], len(out)))
    return out


def _build_sums(g, G, name):
    """groups of G records for the trees (G = 4 x workers per wavefront for the block sums):
      same_point      one point in G different representations: a doubling at every level, G P in the end
      alternating     P, -P, P, -P ...: every first-level addition cancels
      doubling_chain  P, P, 2P, 4P, ...: equal partial sums meet at each higher level
      all_identity    all-zero records and identities with non-zero X, Y
      single          one non-identity record, at each position in turn (the block sums: a spread of positions)
      distinct        distinct random points"""
    rnd = _rng("%d sums %d" % (g, G))
    pts, lams = _point_source(g, "sums %d" % G), _lambda_source(g, "%d sums %d" % (g, G))
    w = FIELDS[g].width
    per = GROUPS_PER_ARRANGEMENT if name == "tree" else BLOCK_CASES_PER_ARRANGEMENT

    def rep(pt):
        return identity_record(g, rnd if rnd.randrange(2) else None) if pt is None else represent(g, pt, next(lams), rnd.randrange(1 << (4 * w)))

    def group(cls, points, want):
        return Case(cls, [rep(pt) for pt in points], None, want)

    blocks = {c: [] for c in ARRANGEMENTS}
    pool = subgroup_points(g)
    for k in range(per):
        p = next(pts)
        blocks["same_point"].append(group("same_point", [p] * G, mul(g, p, G)))
        blocks["alternating"].append(group("alternating", [p if i % 2 == 0 else neg(g, p) for i in range(G)], None))
        chain, total = [p, p], dbl(g, p)
        while len(chain) < G:
            chain.append(total)
            total = dbl(g, total)
        blocks["doubling_chain"].append(group("doubling_chain", chain[:G], total))
        blocks["all_identity"].append(group("all_identity", [None] * G, None))
        chosen = [pool[i] for i in rnd.sample(range(len(pool)), G)]        # distinct multiples of the generator
        want = None
        for pt in chosen:
            want = add(g, want, pt)
        blocks["distinct"].append(group("distinct", chosen, want))
    if name == "tree":
        positions = list(range(G)) * ((per + G - 1) // G)
    else:
        pw = G // 4
        spread = sorted({0, 1, pw - 1, pw, pw + 1, 2 * pw - 1, 2 * pw, 3 * pw, 3 * pw + 1, G - 2, G - 1} & set(range(G)))
        positions = spread + [rnd.randrange(G) for _ in range(per - len(spread))]
    for pos in positions:
        p = next(pts)
        blocks["single"].append(group("single", [p if i == pos else None for i in range(G)], p))
    # interleaved first (one group of each arrangement in turn), then each arrangement's remaining groups in a row
    out = []
    head = min(len(b) for b in blocks.values()) // 2
    for k in range(head):
        out += [blocks[c][k] for c in ARRANGEMENTS]
    for c in ARRANGEMENTS:
        out += blocks[c][head:]
    return out


# the number of cases of every table: a filter that crept into a builder shows here
TABLE_SIZES = {
    "g1-add": 1345, "g1-add_alias": 1345, "g1-madd": 1345, "g1-madd_prefetch": 1345, "g1-dbl": 769, "g1-dbl_affine": 193,
    "g1-from_affine": 385, "g1-to_affine": 577, "g1-is_identity": 577, "g1-tree-G2": 144, "g1-tree-G4": 144,
    "g1-tree-G8": 144, "g1-tree-G16": 152, "g1-tree-G32": 152, "g1-tree-G64": 184, "g1-block_sum": 384, "g1k2-add": 1345,
    "g1k2-add_alias": 1345, "g1k2-load_store": 577, "g1k2-tree-G2": 144, "g1k2-tree-G4": 144, "g1k2-tree-G8": 144,
    "g1k2-tree-G16": 152, "g1k2-tree-G32": 152, "g1k2-block_sum": 384, "g2-add": 1345, "g2-add_alias": 1345,
    "g2-madd": 1345, "g2-madd_prefetch": 1345, "g2-dbl": 769, "g2-dbl_affine": 193, "g2-from_affine": 385,
    "g2-to_affine": 577, "g2-is_identity": 577, "g2-tree-G2": 144, "g2-tree-G4": 144, "g2-tree-G8": 144,
    "g2-tree-G16": 152, "g2-tree-G32": 152, "g2-tree-G64": 184, "g2-block_sum": 384, "g2k3-add": 1345,
    "g2k3-add_alias": 1345, "g2k3-madd": 1345, "g2k3-madd_prefetch": 1345, "g2k3-dbl": 769, "g2k3-dbl_affine": 193,
    "g2k3-from_affine": 385, "g2k3-is_identity": 577, "g2k3-tree-G2": 144, "g2k3-tree-G4": 144, "g2k3-tree-G8": 144,
    "g2k3-tree-G16": 152, "g2k3-block_sum": 384, "g2pair-add": 1345, "g2pair-add_alias": 1345, "g2pair-madd": 1345,
    "g2pair-madd_prefetch": 1345, "g2pair-dbl": 769, "g2pair-dbl_affine": 193, "g2pair-from_affine": 385,
    "g2pair-is_identity": 577, "g2pair-tree-G2": 144, "g2pair-tree-G4": 144, "g2pair-tree-G8": 144,
    "g2pair-tree-G16": 152, "g2pair-tree-G32": 152, "g2pair-block_sum": 384, "g2k6-add": 1345, "g2k6-add_alias": 1345,
    "g2k6-load_store": 577, "g2k6-tree-G2": 144, "g2k6-tree-G4": 144, "g2k6-tree-G8": 144, "g2k6-block_sum": 384,
}


# --------------------------------------------------------------------------------------------- the hooks through ctypes
def shape(lib, form, op):
    out = (ctypes.c_size_t * 4)()
    assert lib.bh_test_group_ops_shape(form, op, out) == 0, (form, op)
    return tuple(int(x) for x in out)     # XYZZ record bytes, flag words per worker, affine record bytes, workers per wavefront


def _pack(records):
    """flat records of equal length -> an (n, 48 * len) byte array"""
    data = b"".join(v.to_bytes(48, "little") for rec in records for v in rec)
    return np.frombuffer(data, dtype=np.uint8).reshape(len(records), -1).copy()


def operand_arrays(form, op, table):
    """(a, b) byte arrays of one table (None where the operation takes none)"""
    name = OPS[op]
    if name in ("tree", "block_sum"):
        return _pack([rec for c in table for rec in c.a]), None
    a = None if name in NO_A else _pack([c.a for c in table])
    b = _pack([c.b for c in table]) if name in B_XYZZ + B_AFFINE else None
    return a, b


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _unpack(raw, n):
    words = raw.reshape(n, -1)
    return [tuple(int.from_bytes(row[i:i + 48].tobytes(), "little") for i in range(0, words.shape[1], 48)) for row in words]


def run_host(lib, form, op, G, table):
    """through bh_test_group_ops_host (forms 0 and 2); for a block sum G = the workers per wavefront to fold by"""
    rbytes = shape(lib, form, op)[0]
    a, b = operand_arrays(form, op, table)
    n = len(table)
    raw = np.zeros((n, rbytes), dtype=np.uint8)
    flags = np.full((n, 1), 0xFFFFFFFF, dtype=np.uint32)
    assert lib.bh_test_group_ops_host(form, op, G, _ptr(raw), _ptr(flags), _ptr(a), _ptr(b), n) == 0, case_id((form, op, G))
    return _unpack(raw, n), flags


GUARD = 4096


def run_dev(lib, worker, form, op, G, table):
    """through bh_test_group_ops_dev; the result and flag arrays are followed by guard bytes that must come back untouched"""
    rbytes, lanes = shape(lib, form, op)[:2]
    a, b = operand_arrays(form, op, table)
    n = len(table)
    raw = np.zeros(n * rbytes + GUARD, dtype=np.uint8)
    raw[n * rbytes:] = 0xA5
    flags = np.full(n * lanes + GUARD // 4, 0xA5A5A5A5, dtype=np.uint32)
    bufs = []
    try:
        dev = []
        for arr in (a, b, raw, flags):
            if arr is None:
                dev.append(None)
                continue
            d = worker.alloc(max(arr.nbytes, 16))
            bufs.append(d)
            worker.upload(d, arr)
            dev.append(d)
        assert lib.bh_test_group_ops_dev(worker.ctx, form, op, G, dev[2], dev[3], dev[0], dev[1], n) == 0, case_id((form, op, G))
        worker.download(raw, dev[2])
        worker.download(flags, dev[3])
    finally:
        for d in bufs:
            worker.free(d)
    assert (raw[n * rbytes:] == 0xA5).all(), "%s: bytes after the %d results were written" % (case_id((form, op, G)), n)
    assert (flags[n * lanes:] == 0xA5A5A5A5).all(), "%s: words after the %d flags were written" % (case_id((form, op, G)), n)
    return _unpack(raw[:n * rbytes], n), flags[:n * lanes].reshape(n, lanes)


# --------------------------------------------------------------------------------------------------------- expectations
def canonical(rec):
    return tuple(v % P for v in rec)


def is_identity_record(g, rec):
    w = FIELDS[g].width
    return all(v % P == 0 for v in rec[2 * w:3 * w])


def check(form, op, G, table, res, flags):
    """assert what the raw results and flags of one (form, op, G) must be - exactly, no tolerances; returns the number of
    cases verified"""
    g, name, lanes = GROUP[form], OPS[op], LANES[form]
    w = FIELDS[g].width
    assert len(res) == len(table) and flags.shape == (len(table), lanes)
    done = 0
    for i, (c, r) in enumerate(zip(table, res)):
        ctx = (case_id((form, op, G)), i, c.cls, "worker %d of its wavefront" % (i % ELEMENT_PER_WAVE[form]), [hex(v) for v in r])
        fl = [int(x) for x in flags[i]]
        assert all(0 <= v < 2 * P for v in r), ctx                                 # every coordinate in [0, 2p)
        if name == "to_affine":
            want_rec = affine_record(g, c.want) + (0,) * (2 * w)                    # canonical x, y; all zero for the identity
            assert r == want_rec and fl == [1 if c.want is None else 0], ctx
            done += 1
            continue
        got = decode(g, r, strict=False)
        assert got != "inconsistent", ctx                                          # ZZ^3 = ZZZ^2
        assert (got is None) == (c.want is None), ctx
        assert got == c.want, ctx
        assert [f & 1 for f in fl] == [1 if c.want is None else 0] * lanes, ctx    # the same answer in every lane
        if name in ("is_identity", "load_store"):
            assert r == c.a, ctx
        if name in ("add", "add_alias", "madd", "madd_prefetch") and c.cls not in ("general", "same", "opposite"):
            # an identity operand means a copy: of b (the affine record with ZZ = ZZZ = 1) or of a
            if is_identity_record(g, c.a):
                copy = c.b if name in B_XYZZ else (c.b + ((ONE,) + (0,) * (w - 1)) * 2 if any(c.b) else c.a)
            else:
                copy = c.a
            assert r == copy, ctx
        if name == "from_affine":
            assert r == (c.b + ((ONE,) + (0,) * (w - 1)) * 2 if c.want is not None else (0,) * (4 * w)), ctx
        if c.cls == "opposite" or (name == "dbl" and c.want is None):
            assert r == (0,) * (4 * w), ctx                                        # xyzz_set_identity
        if name in ("madd", "madd_prefetch"):
            added = not is_identity_record(g, c.a) and any(c.b)
            assert [(f >> 1) & 1 for f in fl] == [1 if added else 0] * lanes, ctx   # what xyzz_madd returned
        if name == "madd_prefetch":
            # the functor ran exactly once on every path and loaded the first word of the worker's own base
            assert [(f >> 4) & 15 for f in fl] == [1] * lanes and [f >> 16 for f in fl] == [c.b[0] & 0xFFFF] * lanes, ctx
        else:
            assert all(f >> 2 == 0 for f in fl), ctx
        done += 1
    return done


def check_against_host(case, table, res, host_res, exact):
    """device against the host build of the same header: every raw limb for the one-lane forms (the representative is
    deterministic), the canonicalised coordinates for the lane forms - they evaluate the same add-2008-s / dbl-2008-s
    formulas with the same projective scaling, so a wrong exchange that still lands on a valid point shows here"""
    for i, (r, h) in enumerate(zip(res, host_res)):
        same = r == h if exact else canonical(r) == canonical(h)
        assert same, (case_id(case), i, table[i].cls, [hex(v) for v in r], [hex(v) for v in h])
    return len(res)
