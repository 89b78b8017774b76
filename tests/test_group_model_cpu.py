"""The integer model of the group law (tests/group_model.py) pinned on its own, the conditions its raw-operand tables
promise, and the tables of the one-lane forms run through the HOST build of csrc/ec.cuh (bh_test_group_ops_host): tables
and expectations are validated without a GPU before tests/test_gpu_group_law.py shows them to one.  No GPU needed."""

import ctypes
import os
import random
from collections import Counter

import numpy as np
import pytest

from bellman_amd import _lib
from oracle import cref
from oracle.pyref import bls12_381 as bls

from tests import field_model as fm
from tests import group_model as gm

P = gm.P


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("g", [1, 2])
def test_model_matches_the_oracles_group_law(g):
    """add / double / multiply against oracle/pyref's affine curve on subgroup AND special points, and against oracle/c
    (cref.point_add / cref.point_mul) on affine records"""
    curve = bls.G1 if g == 1 else bls.G2
    rnd = random.Random(11)
    pts = gm.subgroup_points(g)[:40] + gm.special_points(g) + [None]
    for _ in range(60):
        a, b = rnd.choice(pts), rnd.choice(pts)
        assert gm.add(g, a, b) == curve.add(a, b) and gm.dbl(g, a) == curve.double(a) and gm.neg(g, a) == curve.neg(a)
        assert gm.on_curve(g, gm.add(g, a, b))
    k = rnd.randrange(1 << 70)
    assert gm.mul(g, gm.GEN[g], k) == curve.mul(curve.gen, k)
    to_rec, from_rec = (cref.g1_from_py, cref.g1_to_py) if g == 1 else (cref.g2_from_py, cref.g2_to_py)
    sub = gm.subgroup_points(g)
    for _ in range(20):
        a, b = rnd.choice(sub), rnd.choice(sub + [None])
        ra, rb = to_rec([a])[0], to_rec([b])[0]
        assert from_rec(cref.point_add(g, ra, rb))[0] == gm.add(g, a, b)
        assert from_rec(cref.point_add(g, ra, ra))[0] == gm.dbl(g, a)
    k = rnd.randrange(bls.Q)
    assert from_rec(cref.point_mul(g, to_rec([sub[3]])[0], k))[0] == gm.mul(g, sub[3], k)


def test_model_special_points():
    assert gm.special_points(1) == [(0, 2), (0, P - 2)]
    assert gm.mul(1, (0, 2), 3) is None and gm.dbl(1, (0, 2)) == (0, P - 2)        # order 3
    g2 = gm.special_points(2)
    assert [pt[0] for pt in g2] == [(2, 0), (2, 0), (0, 1), (0, 1)]
    assert not fm.f2_is_square(bls.G2_B)                                           # no point of the twist has x = 0
    for g in (1, 2):
        for pt in gm.special_points(g):
            assert gm.on_curve(g, pt) and gm.mul(g, pt, bls.Q) is not None          # on the curve, off the subgroup
    assert all(gm.on_curve(g, pt) for g in (1, 2) for pt in gm.subgroup_points(g))
    assert gm.mul(2, gm.GEN[2], bls.Q) is None


@pytest.mark.parametrize("g", [1, 2])
def test_model_representations_decode(g):
    """every representation of a point decodes to the point, whatever l and whichever coefficients carry + p"""
    rnd = random.Random(5)
    lams = gm._lambda_source(g, "decode")
    w = gm.FIELDS[g].width
    for pt in gm.subgroup_points(g)[:20] + gm.special_points(g):
        for _ in range(3):
            rec = gm.represent(g, pt, next(lams), rnd.randrange(1 << (4 * w)))
            assert all(0 <= v < 2 * P for v in rec) and gm.decode(g, rec) == pt
    assert gm.decode(g, gm.identity_record(g)) is None and gm.decode(g, gm.identity_record(g, rnd)) is None
    bad = list(gm.represent(g, gm.GEN[g], next(lams), 0))
    bad[-1] ^= 1
    assert gm.decode(g, tuple(bad), strict=False) == "inconsistent"


# ----------------------------------------------------------------------------------------------------------- the tables
def _scale(g, rec):
    """(ZZ, ZZZ) in [0, p): one l, one pair"""
    w = gm.FIELDS[g].width
    return tuple(v % P for v in rec[2 * w:])


def _class_of(g, name, c):
    """the class of a case re-derived from its records through the model alone"""
    base = {"add_alias": "add", "madd_prefetch": "madd"}.get(name, name)
    w = gm.FIELDS[g].width
    dirty = lambda rec: gm.is_identity_record(g, rec) and any(rec[:2 * w])      # noqa: E731
    if base in ("add", "madd"):
        pa = gm.decode(g, c.a)
        pb = gm.decode(g, c.b) if base == "add" else (None if not any(c.b) else fm.real(fm.shaped((gm.FIELDS[g].zero,) * 2, iter(c.b))))
        if dirty(c.a) or (base == "add" and dirty(c.b)):
            return "dirty_identity", gm.add(g, pa, pb)
        return gm.classify(g, pa, pb), gm.add(g, pa, pb)
    if base in ("dbl_affine", "from_affine"):
        pt = None if not any(c.b) else fm.real(fm.shaped((gm.FIELDS[g].zero,) * 2, iter(c.b)))
        return ("general" if pt is not None else "b_identity"), (gm.dbl(g, pt) if base == "dbl_affine" else pt)
    pt = gm.decode(g, c.a, strict=False)
    if pt == "inconsistent" or (pt is not None and all(v % P == 0 for v in c.a[w:2 * w])):
        return "y_zero", None
    cls = "general" if pt is not None else "dirty_identity" if dirty(c.a) else "a_identity"
    return cls, (gm.dbl(g, pt) if base == "dbl" else pt)


ELEMENT_TABLES = sorted({(gm.GROUP[f], gm.OPS[op]) for f, op, G in gm.cases() if gm.OPS[op] not in ("tree", "block_sum")})


@pytest.mark.parametrize("g,name", ELEMENT_TABLES, ids=["g%d-%s" % t for t in ELEMENT_TABLES])
def test_element_tables_hold_what_they_promise(g, name):
    form = 0 if g == 1 else 2
    if name == "load_store":
        form += 1 if g == 1 else 3
    table = gm.operands_for((form, gm.OP[name], 0))
    classes = gm.CLASSES[name]
    w = gm.FIELDS[g].width
    # the class and the expected point of every case follow from its records through the model alone
    for c in table:
        cls, want = _class_of(g, name, c)
        assert (cls, want) == (c.cls, c.want)
        for rec in (c.a, c.b):
            assert rec is None or all(0 <= v < 2 * P for v in rec)
    count = Counter(c.cls for c in table)
    assert set(count) == set(classes) and all(count[c] >= 64 + gm.PER_CLASS_RUN for c in classes)
    # every raw record that is a point has an l of its own
    scales = [_scale(g, rec) for c in table for rec in ((c.a, c.b) if name in gm.B_XYZZ else (c.a,))
              if rec is not None and not gm.is_identity_record(g, rec)]
    assert len(scales) == len(set(scales))
    # same / opposite points: different l AND different representatives on the two sides
    if name in gm.B_XYZZ:
        for c in table:
            if c.cls in ("same", "opposite"):
                assert _scale(g, c.a) != _scale(g, c.b) and [v >= P for v in c.a] != [v >= P for v in c.b]
        zz = Counter(rec[2 * w] for c in table if c.cls == "dirty_identity" for rec in (c.a, c.b) if gm.is_identity_record(g, rec))
        assert zz[0] >= 32 and zz[P] >= 32                                          # ZZ written as 0 and as p
    # interleaved: the first 64 rounds change class from worker to worker; homogeneous: a whole wavefront of every form
    # takes one branch; ragged: no form's last wavefront is full
    head = table[:gm.PER_CLASS_INTERLEAVED * len(classes)]
    if len(classes) > 1:
        assert all(x.cls != y.cls for x, y in zip(head, head[1:]))
    for f in (f for f in gm.FORMS if gm.GROUP[f] == g and name in gm.form_ops(f)):
        pw = gm.ELEMENT_PER_WAVE[f]
        waves = [set(c.cls for c in table[k:k + pw]) for k in range(0, len(table) - pw + 1, pw)]
        assert {next(iter(s)) for s in waves if len(s) == 1} == set(classes)
        assert len(table) % pw
        assert len(table) == gm.TABLE_SIZES[gm.case_id((f, gm.OP[name], 0))]


@pytest.mark.parametrize("g", [1, 2])
def test_sum_tables_hold_what_they_promise(g):
    per_form = {f: Counter() for f in gm.FORMS if gm.GROUP[f] == g}
    for form, op, G in gm.cases():
        if gm.GROUP[form] != g or gm.OPS[op] not in ("tree", "block_sum"):
            continue
        table = gm.operands_for((form, op, G))
        width = G if G else 4 * gm.TREE_PER_WAVE[form]
        assert len(table) == gm.TABLE_SIZES[gm.case_id((form, op, G))]
        count = Counter(c.cls for c in table)
        assert set(count) == set(gm.ARRANGEMENTS)
        if gm.OPS[op] == "tree":
            per_form[form].update(count)
            assert all(n >= gm.GROUPS_PER_ARRANGEMENT for n in count.values())
        else:
            assert all(n >= 64 for n in count.values())
        singles = set()
        for c in table:
            assert len(c.a) == width
            pts = [gm.decode(g, rec) for rec in c.a]
            total = None
            for pt in pts:
                total = gm.add(g, total, pt)
            assert total == c.want
            live = [i for i, pt in enumerate(pts) if pt is not None]
            if c.cls == "same_point":
                assert len(set(pts)) == 1 and len({_scale(g, rec) for rec in c.a}) == width
            elif c.cls == "alternating":
                assert all(pts[i] == gm.neg(g, pts[i + 1]) for i in range(0, width, 2)) and c.want is None
            elif c.cls == "doubling_chain":
                assert pts[0] == pts[1] and all(pts[i] == gm.dbl(g, pts[i - 1]) for i in range(2, width))
            elif c.cls == "all_identity":
                assert not live
            elif c.cls == "single":
                assert len(live) == 1
                singles.add(live[0])
            else:
                assert len(set(pts)) == width and None not in pts
        if gm.OPS[op] == "tree":
            assert singles == set(range(G))                                        # at each position in turn
        else:
            pw = width // 4
            assert {0, pw - 1, pw, 2 * pw, 3 * pw, width - 1} <= singles
    for form, count in per_form.items():
        assert all(count[c] >= 64 for c in gm.ARRANGEMENTS), (form, count)         # over the widths of one form


# ------------------------------------------------------------------------------------------------------- the host twins
HOST_CASES = [case for case in gm.cases() if case[0] in (0, 2)]


@pytest.mark.parametrize("case", HOST_CASES, ids=gm.case_id)
def test_host_build_on_raw_operands(lib, case):
    """one form x operation of the host build over its whole table against the integer model, then one case on its own"""
    form, op, G = case
    table = gm.operands_for(case)
    res, flags = gm.run_host(lib, form, op, G, table)
    assert gm.check(form, op, G, table, res, flags) == len(table) == gm.TABLE_SIZES[gm.case_id(case)]
    for k in (0, len(table) // 2):
        res1, flags1 = gm.run_host(lib, form, op, G, table[k:k + 1])
        assert gm.check(form, op, G, table[k:k + 1], res1, flags1) == 1 and res1[0] == res[k]


LANE_SUM_CASES = [case for case in gm.cases() if case[0] in (1, 3, 4, 5) and gm.OPS[case[1]] == "block_sum"]


@pytest.mark.parametrize("case", LANE_SUM_CASES, ids=gm.case_id)
def test_host_block_sums_in_the_order_of_the_lane_forms(lib, case):
    """the block-sum tables of the lane forms (4 x 32, 16 or 8 records) through the host build folding by that many
    workers per wavefront: what the device forms are compared with"""
    form = case[0]
    host_form = 0 if gm.GROUP[form] == 1 else 2
    table = gm.operands_for(case)
    res, flags = gm.run_host(lib, host_form, case[1], gm.TREE_PER_WAVE[form], table)
    assert gm.check(host_form, case[1], 0, table, res, flags) == len(table)


def test_group_hook_rejects_what_it_does_not_know(lib):
    out = np.zeros(4096, dtype=np.uint8)
    fl = np.zeros(16, dtype=np.uint32)
    p, f = out.ctypes.data, fl.ctypes.data
    host = lib.bh_test_group_ops_host
    assert host(1, 0, 0, p, f, p, p, 1) != 0 and host(3, 0, 0, p, f, p, p, 1) != 0     # lane forms: device only
    assert host(0, 9, 0, p, f, p, p, 1) != 0 and host(0, 12, 0, p, f, p, p, 1) != 0    # load_store, an unknown operation
    assert host(0, 0, 0, p, f, p, None, 1) != 0 and host(0, 4, 0, p, f, None, None, 1) != 0   # a missing operand
    assert host(0, 10, 3, p, f, p, None, 1) != 0 and host(0, 10, 128, p, f, p, None, 1) != 0 and host(0, 10, 1, p, f, p, None, 1) != 0
    assert host(6, 0, 0, p, f, p, p, 1) != 0
    shape = (ctypes.c_size_t * 4)()
    assert lib.bh_test_group_ops_shape(3, 7, shape) != 0 and lib.bh_test_group_ops_shape(1, 2, shape) != 0
    assert [gm.shape(lib, form, 0) for form in gm.FORMS] == [(192, 1, 96, 64), (192, 2, 96, 32), (384, 1, 192, 64),
                                                             (384, 3, 192, 16), (384, 2, 192, 32), (384, 6, 192, 8)]
