"""tests/models/pairing_stage_model.py pinned without a GPU: its Miller value against oracle/pyref and against the host
build of csrc/fp12.cuh, its window table and digits against plain scalar multiplication, its verdict against the shipped
proof_status_error, and the conditions tests/test_gpu_pairing_stages.py relies on in the operand tables."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bellman_amd import _lib  # noqa: E402
from tests import field_model as fm  # noqa: E402
from tests import group_model as gm  # noqa: E402
from tests.models import pairing_stage_model as psm  # noqa: E402
from tests.test_verifier_cpu import host_pairings, pyref_pairing_cubed  # noqa: E402

P, Q = psm.P, psm.Q


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libbellman_hip_test.so not built")
    return _lib.load()


@pytest.fixture(scope="module")
def pairs():
    rnd = psm.rng("pins")
    g1, g2 = gm.GEN[1], gm.GEN[2]
    return [(g1, g2)] + [(gm.mul(1, g1, rnd.randrange(1, Q)), gm.mul(2, g2, rnd.randrange(1, Q))) for _ in range(2)]


def _model_gt(p, q):
    """The head of csrc/fp12.cuh: the loop runs over |x| WITHOUT the final conjugation, and the final exponentiation is
    f^(3 (p^12 - 1) / q).  oracle/pyref/pairing.py loops over |x| without a conjugation too, with affine lines that differ
    from the projective ones by subfield factors, and raises to (p^12 - 1) / q: so the model's Miller value, raised through
    the oracle's exponent and cubed, is the oracle's pairing cubed, coefficient for coefficient - no conjugate is taken on
    either side (tests/test_verifier_cpu.py::test_host_pairing_matches_pyref pins the host build the same way)."""
    return fm.f12_to_wbasis(fm.f12_pow(psm.miller(p, q), fm.FINAL_EXP))


def test_model_miller_value_against_the_oracle(pairs):
    for p, q in pairs:
        assert _model_gt(p, q) == pyref_pairing_cubed(p, q)


def test_model_miller_value_against_the_host_build(lib, pairs):
    for (p, q), got in zip(pairs, host_pairings(lib, pairs)):
        assert _model_gt(p, q) == got
    assert psm.miller(None, pairs[0][1]) == fm.F12_ONE and psm.miller(pairs[0][0], None) == fm.F12_ONE


def test_shared_squarings_give_the_product_of_the_loops(pairs):
    each = [psm.miller(p, q) for p, q in pairs]
    assert psm.miller_multi([(p, psm.g2_lines(q)) for p, q in pairs]) == psm.f12_product(each)


def test_lines_are_those_of_the_negated_point_under_negate():
    q = gm.GEN[2]
    lines, neg = psm.g2_lines(q), psm.g2_lines(gm.neg(2, q))
    assert lines != neg and len(lines) == psm.MILLER_LINES
    p = gm.GEN[1]
    f, g = psm.miller_loop_lines(p, lines), psm.miller_loop_lines(p, neg)
    one = fm.f12_pow(fm.f12_mul(f, g), fm.FINAL_EXP)
    assert one == fm.F12_ONE                                   # e(P, Q) e(P, -Q) = 1


@pytest.mark.parametrize("w", psm.WIDTHS)
def test_table_model_is_plain_scalar_multiplication(w):
    pts = [gm.GEN[1], (0, 2), None, psm.g1_points()["random"][0]]
    table = psm.ic_table(pts, w)
    windows, entries = psm.table_shape(w)
    assert len(table) == len(pts) and all(len(rows) == windows and all(len(r) == entries for r in rows) for rows in table)
    rnd = psm.rng("table %d" % w)
    probes = {(0, 0), (windows - 1, entries - 1), (windows - 1, 0), (1, entries - 1)} | {
        (rnd.randrange(windows), rnd.randrange(entries)) for _ in range(6)}
    for i, pt in enumerate(pts):
        for win, e in probes:
            want = None if pt is None else gm.mul(1, pt, (e + 1) << (w * win))
            assert table[i][win][e] == want, (w, i, win, e)
    assert psm.table_bytes(16, w) == 16 * windows * entries * 96


@pytest.mark.parametrize("w", psm.WIDTHS)
def test_digits_reassemble_the_scalar(w):
    rnd = psm.rng("digits")
    windows, entries = psm.table_shape(w)
    for k in list(psm.FR_EDGES) + [rnd.randrange(1 << 256) for _ in range(20)]:
        d = psm.digits(k, w)
        assert len(d) == windows and all(0 <= x <= entries for x in d)
        assert sum(x << (w * win) for win, x in enumerate(d)) == k
    assert psm.digits((1 << 256) - 1, w) == [entries] * windows


def test_accumulation_by_table_terms_is_the_affine_sum():
    pts = [gm.GEN[1], psm.g1_points()["random"][1], None]
    ic0 = psm.g1_points()["random"][2]
    for w in psm.WIDTHS:
        table = psm.ic_table(pts, w)
        for scalars in ((1, Q - 1, 5), (Q, (1 << 256) - 1, 1), (0, 0, 0)):
            assert psm.g1_sum(psm.accumulate_terms(table, w, scalars) + [ic0]) == psm.ic_accumulate(ic0, pts, scalars)


def test_verdict_model_against_proof_status_error(lib):
    for s in range(256):
        for pos in range(3):
            word = s << (8 * pos)
            assert psm.status_error(word) == lib.bh_test_proof_status_error(word), (s, pos)
            # ... behind an infinity and behind an invalid element in an earlier position
            for first in (psm.PT_IS_INF, 32):
                if pos:
                    both = word | first
                    assert psm.status_error(both) == lib.bh_test_proof_status_error(both), (s, pos, first)
            assert psm.verdict(word, 0, 0, 1) == psm.status_error(word)
    assert psm.verdict(None, 0, 0, 1) == psm.OK and psm.verdict(None, 0, 0, 0) == psm.INVALID_PROOF
    assert psm.verdict(None, 0, 0, 2) == psm.INVALID_PROOF
    assert psm.verdict(0, 2, 0, 0) == psm.INVALID_POINT and psm.verdict(0, 0, 3, 1) == psm.INVALID_POINT
    assert psm.verdict(0, 0, 1, 1) == psm.OK
    assert psm.verdict(psm.PT_IS_INF, 2, 2, 0) == psm.POINT_AT_INFINITY


def test_colsum_model_is_the_plain_sum():
    rnd = psm.rng("colsum model")
    n, ncol = 700, 3
    z = [rnd.randrange(1, 1 << 256) for _ in range(n)]
    rows = [[rnd.randrange(1 << 256) for _ in range(ncol - 1)] for _ in range(n)]
    acc0 = [rnd.randrange(Q) for _ in range(ncol)]
    for nb in (psm.colsum_nb(n), 1):
        part, acc = psm.colsum(z, rows, ncol, acc0, psm.CANONICAL, nb)
        assert acc[0] == (acc0[0] + sum(z)) % Q
        assert acc[2] == (acc0[2] + sum(a * r[1] for a, r in zip(z, rows))) % Q
        assert all(len(p) == nb for p in part)
    assert psm.colsum_nb(1) == 1 and psm.colsum_nb(257) == 2 and psm.colsum_nb(16384) == 64 and psm.colsum_nb(16383) == 64


# ------------------------------------------------------------------------------------------- what the GPU file relies on
def test_g1_operand_classes():
    cls = psm.g1_points()
    assert set(cls) == {"generator", "random", "order3", "off_subgroup", "off_curve", "identity"}
    for name in ("generator", "random"):
        assert all(gm.on_curve(1, pt) and gm.mul(1, pt, Q) is None for pt in cls[name])
    assert cls["order3"] == [(0, 2), (0, P - 2)]
    assert all(gm.on_curve(1, pt) and gm.mul(1, pt, 3) is None and gm.mul(1, pt, 2) == gm.neg(1, pt) for pt in cls["order3"])
    assert all(gm.on_curve(1, pt) and gm.mul(1, pt, Q) is not None for pt in cls["off_subgroup"])
    assert all(not gm.on_curve(1, pt) for pt in cls["off_curve"]) and (P - 1, P - 1) in cls["off_curve"]
    assert cls["identity"] == [None]
    # [z] A for z >= q on a point outside the subgroup differs from [z mod q] A: the integer is what counts
    a = cls["off_subgroup"][0]
    assert psm.g1_mul(a, Q + 1) != a and psm.g1_mul(a, (1 << 256) - 1) != psm.g1_mul(a, ((1 << 256) - 1) % Q)


def test_g2_operand_classes():
    cls = psm.g2_points()
    assert set(cls) == {"generator", "random", "x_c1_zero", "x_c0_zero", "off_subgroup", "off_curve", "identity"}
    assert all(len(v) >= 1 for v in cls.values())
    for name in ("generator", "random"):
        assert all(gm.on_curve(2, pt) and gm.mul(2, pt, Q) is None for pt in cls[name])
    assert all(gm.on_curve(2, pt) and pt[0][1] == 0 and pt[0][0] != 0 for pt in cls["x_c1_zero"])
    assert all(gm.on_curve(2, pt) and pt[0][0] == 0 and pt[0][1] != 0 for pt in cls["x_c0_zero"])
    assert all(gm.on_curve(2, pt) and gm.mul(2, pt, Q) is not None for pt in cls["off_subgroup"])
    assert all(not gm.on_curve(2, pt) for pt in cls["off_curve"])


def test_lane_plan_puts_every_class_at_the_hot_lanes():
    for classes in (psm.g1_points(), psm.g2_points()):
        for n in (1, 63, 64, 65, 129):
            plan, rotations = psm.lane_plan(classes, n)
            seen = {lane: set() for lane in (0, 63, 64) if lane < n}
            for rot in range(rotations):
                picks = plan(rot)
                assert len(picks) == n
                for lane in seen:
                    seen[lane].add(picks[lane][0])
            assert all(v == set(classes) for v in seen.values()), n


def test_z_values_cover_the_edges():
    vals, raw = psm.z_values(psm.CANONICAL, 65, "t")
    assert set(psm.Z_EDGES) <= set(vals) and vals == raw and all(v % Q for v in vals)
    vals, raw = psm.z_values(psm.MONT, 65, "t")
    assert {1, 2, Q - 1} <= set(vals) and all(v < Q and r < Q for v, r in zip(vals, raw))
    assert all(psm.scalar_int(r, psm.MONT) == v for v, r in zip(vals, raw))


def test_equal_and_opposite_ic_reach_the_doubling_and_cancellation_branches():
    """ic_2 = ic_1 with inputs (1, 1): the second term meets an accumulator equal to it; ic_2 = -ic_1 with equal inputs: the
    last term meets its opposite and leaves the identity (an all-zero record with an identity ic_0)"""
    ic1 = psm.g1_points()["random"][0]
    for w in psm.WIDTHS:
        same = psm.accumulate_terms(psm.ic_table([ic1, ic1], w), w, (1, 1))
        assert len(same) == 2 and gm.classify(1, same[0], same[1]) == "same"
        a = Q - 1
        terms = psm.accumulate_terms(psm.ic_table([ic1, gm.neg(1, ic1)], w), w, (a, a))
        acc, kinds = None, []
        for t in terms:
            kinds.append(gm.classify(1, acc, t))
            acc = gm.add(1, acc, t)
        assert acc is None and kinds[-1] == "opposite", (w, kinds[-3:])
        assert psm.ic_accumulate(None, [ic1, gm.neg(1, ic1)], (a, a)) is None


def test_scalar_key_proofs_verify_in_the_oracle():
    from oracle.pyref import pairing as pyp

    key = psm.ScalarKey(2, "cpu")
    inputs = [5, Q - 1]
    a, b, c = key.proof(inputs)
    acc = psm.ic_accumulate(key.ic[0], key.ic[1:], inputs)
    e = pyref_pairing_cubed
    assert e(a, b) == pyp.f12_mul(pyp.f12_mul(e(key.alpha, key.beta), e(acc, key.gamma)), e(c, key.delta))
