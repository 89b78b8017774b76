"""The integer model of the fields (tests/field_model.py) pinned on its own, and the corner operand tables of
tests/test_gpu_field_corners.py run through the HOST build of the same headers (bh_test_field_ops_host): the tables and
the expectations are validated without a GPU before a GPU sees them.  No GPU needed."""

import os
import random

import numpy as np
import pytest

from bellman_amd import _lib
from oracle.pyref import pairing as pyref_pairing

from tests import field_model as fm  # noqa: E402

P, Q = fm.P, fm.Q


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _rand(rnd, like):
    return fm.shaped(like, iter([rnd.randrange(P) for _ in range(len(fm.flat(like)))]))


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("zero,one,add,mul,inv", [
    (fm.F2_ZERO, fm.F2_ONE, fm.f2_add, fm.f2_mul, fm.f2_inv),
    (fm.F6_ZERO, fm.F6_ONE, fm.f6_add, fm.f6_mul, fm.f6_inv),
    (fm.F12_ZERO, fm.F12_ONE, lambda a, b: (fm.f6_add(a[0], b[0]), fm.f6_add(a[1], b[1])), fm.f12_mul, fm.f12_inv),
], ids=["fp2", "fp6", "fp12"])
def test_model_field_axioms(zero, one, add, mul, inv):
    rnd = random.Random(2024)
    for _ in range(10):
        a, b, c = _rand(rnd, zero), _rand(rnd, zero), _rand(rnd, zero)
        assert mul(a, b) == mul(b, a) and mul(mul(a, b), c) == mul(a, mul(b, c))
        assert mul(a, add(b, c)) == add(mul(a, b), mul(a, c))
        assert mul(a, one) == a and add(a, zero) == a and mul(a, zero) == zero
        assert mul(a, inv(a)) == one
    assert inv(zero) == zero and inv(one) == one


def test_model_tower_relations():
    """u^2 = -1, v^3 = xi, w^2 = v, and the Montgomery helpers invert each other"""
    assert fm.f2_mul((0, 1), (0, 1)) == (P - 1, 0)
    v = (fm.F2_ZERO, fm.F2_ONE, fm.F2_ZERO)
    assert fm.f6_mul(fm.f6_mul(v, v), v) == (fm.XI, fm.F2_ZERO, fm.F2_ZERO) and fm.f6_mul_v(fm.F6_ONE) == v
    w = (fm.F6_ZERO, fm.F6_ONE)
    assert fm.f12_mul(w, w) == (v, fm.F6_ZERO)
    x = _rand(random.Random(1), fm.F12_ZERO)
    assert fm.real(fm.mont(x)) == x and fm.shaped(x, iter(fm.flat(x))) == x
    assert fm.RP_INV * fm.RP % P == 1 and fm.RQ_INV * fm.RQ % Q == 1


def test_model_matches_pyref_pairing_arithmetic():
    """an independent statement of Fp12 (polynomials in w, oracle/pyref/pairing.py) gives the same products and powers"""
    rnd = random.Random(7)
    for _ in range(5):
        a, b = _rand(rnd, fm.F12_ZERO), _rand(rnd, fm.F12_ZERO)
        assert fm.f12_to_wbasis(fm.f12_mul(a, b)) == pyref_pairing.f12_mul(fm.f12_to_wbasis(a), fm.f12_to_wbasis(b))
        assert fm.f12_from_wbasis(fm.f12_to_wbasis(a)) == a
    e = rnd.randrange(1 << 200)
    assert fm.f12_to_wbasis(fm.f12_pow(a, e)) == pyref_pairing.f12_pow(fm.f12_to_wbasis(a), e)


def test_model_frobenius_is_the_pth_power():
    """frob(x) = x^p, against its structure: the coefficient g_k of w^k goes to conj(g_k) xi^(k (p - 1) / 6), and for p^2
    to g_k xi^(k (p^2 - 1) / 6) with a constant in Fp (the constants of csrc/fp12.cuh, recomputed from p here)"""
    rnd = random.Random(3)
    for _ in range(3):
        x = _rand(rnd, fm.F12_ZERO)
        g = fm.f12_to_wbasis(x)
        f1 = tuple(fm.f2_mul(fm.f2_conj(g[k]), fm.f2_pow(fm.XI, k * (P - 1) // 6)) for k in range(6))
        assert fm.f12_frob(x, 1) == fm.f12_pow(x, P) == fm.f12_from_wbasis(f1)
        c2 = [fm.f2_pow(fm.XI, k * (P * P - 1) // 6) for k in range(6)]
        assert all(c[1] == 0 for c in c2)
        assert fm.f12_frob(x, 2) == fm.f12_from_wbasis(tuple(fm.f2_scale(g[k], c2[k][0]) for k in range(6)))
        assert fm.f12_frob(fm.f12_frob(x, 1), 1) == fm.f12_frob(x, 2)
        y = _rand(rnd, fm.F12_ZERO)
        assert fm.f12_frob(fm.f12_mul(x, y)) == fm.f12_mul(fm.f12_frob(x), fm.f12_frob(y))


def test_model_square_roots():
    rnd = random.Random(5)
    for _ in range(40):
        x = rnd.randrange(P)
        r = fm.fp_sqrt(x * x % P)
        assert r is not None and r * r % P == x * x % P
        assert (fm.fp_sqrt(x) is not None) == fm.fp_is_square(x)
        a = (rnd.randrange(P), rnd.randrange(P))
        sq = fm.f2_mul(a, a)
        r = fm.f2_sqrt(sq)
        assert r is not None and fm.f2_mul(r, r) == sq and fm.f2_is_square(sq)
        r = fm.f2_sqrt(a)
        assert (r is not None) == fm.f2_is_square(a)
        assert r is None or fm.f2_mul(r, r) == a
    assert fm.f2_sqrt((P - 1, 0)) in ((0, 1), (0, P - 1)) and fm.f2_sqrt(fm.F2_ZERO) == fm.F2_ZERO


def test_model_cyclotomic_elements(lib):
    """The operands of f12_cyc_sqr / f12_cyc_exp_x lie in the cyclotomic subgroup - x^(p^4 - p^2 + 1) = 1 and
    conj(x) = 1 / x - which is what makes the Granger-Scott squaring equal the plain square; on an element outside the
    subgroup the host build's cyclotomic squaring does NOT give the square, so the table is not interchangeable."""
    for v in fm.cyclotomic_values():
        x = fm.real(fm.shaped(fm.F12_ZERO, iter(v)))
        assert fm.f12_mul(fm.f12_conj(x), x) == fm.F12_ONE
        assert fm.f12_pow(x, P ** 4 - P ** 2 + 1) == fm.F12_ONE
    outside = fm.mont(_rand(random.Random(9), fm.F12_ZERO))
    raw, _ = fm.run_host(lib, 6, 18, [outside])
    got = fm.real(fm.shaped(fm.F12_ZERO, iter(fm.unpack(raw)[0])))
    assert got != fm.f12_mul(fm.real(outside), fm.real(outside))


# ----------------------------------------------------------------------------------------------------------- the tables
TABLE_SIZES = fm.TABLE_SIZES


def test_corner_tables_hold_what_they_promise():
    c = fm.FP_LAZY
    assert (len(fm.FP_LAZY), len(fm.FP_CANON), len(fm.FR_CANON)) == (153, 149, 101)
    assert all(0 <= v < 2 * P for v in c) and all(v < P for v in fm.FP_CANON) and all(v < Q for v in fm.FR_CANON)
    r = fm.RP % P
    for v in (0, 1, 2, P - 1, P, P + 1, 2 * P - 2, 2 * P - 1, r, r - 1, r + 1, (P + 1) // 2, (P - 1) // 2, (P - 3) // 4):
        assert v in c
    for k in list(range(30, 384, 30)) + list(range(32, 384, 32)):
        for d in (-1, 0, 1):
            assert (1 << (k + d)) in c and (1 << (k + d)) - 1 in c
    limbs30 = [(c[-3] >> (30 * i)) & 0x3FFFFFFF for i in range(13)]
    assert limbs30[:12] == [0x3FFFFFFF] * 12 and c[-3] + (1 << 360) >= 2 * P
    for v, phase in ((c[-2], 0), (c[-1], 1)):
        limbs = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
        top = max(i for i in range(12) if limbs[i])
        assert all(limbs[i] == (0xFFFFFFFF if i % 2 == phase else 0) for i in range(top))
    assert {fm.case_id(case): len(fm.operands_for(case)) for case in fm.cases()} == TABLE_SIZES
    # the pairs built for the branches are there, every one in domain
    pairs = set(fm.operands_for((2, 0)))
    assert {(P, P), (P - 1, P + 1), (2, 2 * P - 2), (2, 2 * P - 3), (2, 2 * P - 1), (0, P), (P, 0), (1, P + 1), (0, 1)} <= pairs
    quads = fm.operands_for((2, 10))
    assert (2 * P - 1,) * 4 in quads and any(q[2] == 0 for q in quads) and any(q[2] == P for q in quads)
    wide = [pq for pq in fm.operands_for((2, 7)) if pq[0] >= 2 * P or pq[1] >= 2 * P]
    n_high = sum(1 for a in fm.HIGH_WIDE for b in fm.HIGH_LAZY if a >= 2 * P) + sum(1 for a in fm.HIGH_WIDE[:20] if a >= 2 * P) * 20
    assert len(wide) == 2 * len(fm.FP_WIDE) * len(c) + n_high                # no wide pair was filtered out
    assert n_high > 3000 and all(((v >> (30 * i)) & 0x3FFFFFFF) >= 0x3FFFFF00 for v in fm.HIGH_LAZY for i in range(12))
    f2 = set(fm.operands_for((3, 9)))
    assert {(P, P), (0, 0), (1, 0), (0, 1), (1, P - 1), (P - 1, P - 1), (2 * P - 1, 0)} <= f2
    for form, per_wave in ((4, 21), (5, 32)):                               # ragged lengths for the lane forms
        for op in fm.LANE_OPS:
            n = len(fm.operands_for((form, op)))
            assert n % 21 and n % 32 and n > 20 * per_wave


# ------------------------------------------------------------------------------------------------------- the host twins
HOST_CASES = [case for case in fm.cases() if case[0] not in (4, 5)]


@pytest.mark.parametrize("case", HOST_CASES, ids=fm.case_id)
def test_host_build_at_corner_operands(lib, case):
    """one form x operation of the host build over its whole operand table, against the integer model: exact limbs for
    the canonical forms, congruence and the documented bound for the lazily reduced ones, the predicates' flags"""
    form, op = case
    operands = fm.operands_for(case)
    raw, flags = fm.run_host(lib, form, op, operands)
    assert fm.check(form, op, operands, raw, flags) == len(operands) == TABLE_SIZES[fm.case_id(case)]


def test_field_hook_rejects_what_it_does_not_know(lib):
    out = np.zeros(576, dtype=np.uint8)
    fl = np.zeros(4, dtype=np.uint32)
    p = out.ctypes.data
    assert lib.bh_test_field_ops_host(4, 0, p, fl.ctypes.data, p, p, None, None, 1) != 0     # lane forms: device only
    assert lib.bh_test_field_ops_host(2, 15, p, fl.ctypes.data, p, p, p, p, 1) != 0
    assert lib.bh_test_field_ops_host(3, 13, p, fl.ctypes.data, p, p, p, p, 1) != 0
    assert lib.bh_test_field_ops_host(2, 0, p, fl.ctypes.data, p, None, None, None, 1) != 0   # a missing operand
    assert lib.bh_test_field_ops_host(9, 0, p, fl.ctypes.data, p, p, None, None, 1) != 0
