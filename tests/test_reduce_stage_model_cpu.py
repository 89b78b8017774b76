"""Stage 5 of a multiexp and its host tail without a GPU (bh_test_reduce_plan and bh_test_msm_host_tail are host code):

  the plan      every launch the shipped launch_reduce issues - the schedule that reduce_plan returns and launch_reduce
                walks - replayed over integer buckets by tests/models/reduce_stage_model.py, for every c in [2, 24] x both plan
                kinds x the three bundles msm_enqueue reduces with x 32, 64, 128 and 256 compute units (an MI355X in a
                partitioned compute mode reports the smaller counts and then takes other branches);
  coverage      the matrix must reach every worker kind and workgroup width, both sides of every switch (asserted);
  the host tail msm_host_tail<FpOps / Fp2Ops> over records of the test's choice - fresh scalings, coordinates as v or v + p,
                both forms of the identity, equal and opposite points where `acc` and `u` meet - against Python integers."""
import ctypes
import random

import numpy as np
import pytest

from oracle.pyref import bls12_381 as bls
from tests import group_model as gm
from tests.models import reduce_stage_model as rsm

CS = range(2, 25)
NUM_CUS = (32, 64, 128, 256)


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load().test


# --------------------------------------------------------------------------------------------------------------- the plan
_coverage, _replayed = {}, {}


@pytest.mark.parametrize("kind", sorted(rsm.KINDS), ids=lambda k: rsm.KINDS[k])
@pytest.mark.parametrize("form", sorted(rsm.FORMS), ids=lambda f: rsm.FORMS[f])
def test_recorded_launches_over_integers(lib, form, kind):
    facts = set()
    for c in CS:
        for num_cus in NUM_CUS:
            plan, launches = rsm.query(lib, form, kind, c, num_cus)
            W = -(-256 // c) if kind == 0 else 1
            assert (plan["c"], plan["W"], plan["nb"], plan["NB"]) == (c, W, 1 << (c - 1), W << (c - 1)), plan
            assert plan["lo_bits"] == (c - 1) // 2 and plan["lo_bits"] + plan["hi_bits"] == c - 1, plan
            assert plan["rowcol"] == W * ((1 << plan["lo_bits"]) + (1 << plan["hi_bits"])) and plan["bits"] == W * c, plan
            assert plan["record"] == 4 * 48 * gm.FIELDS[rsm.FORM_GROUP[form]].width, plan
            # the replay depends on what the jobs read and write, not on the lanes and workers that do it: one replay for
            # the bundles and chip sizes that agree on that (the shapes are checked for every one)
            key = (kind, c, rsm.access_key(launches))
            if key not in _replayed:
                _replayed[key] = rsm.check_plan(plan, launches, rsm.seeded_buckets(dict(plan, form=0), 5))[:2]
            else:
                rsm.check_shapes(plan, launches)
            rsm.check_written_once(plan, _replayed[key][1])   # this plan's own sizes and want_part against what is written
            facts |= rsm.coverage(plan, launches)
    _coverage[(form, kind)] = facts
    # the two-stage rule's edges: NB = 2^17 and 2^21 inside, one step outside not
    if kind == 1 and form in (0, 1):
        for c, want in ((17, 0), (18, 1), (22, 1), (23, 0)):
            assert rsm.query(lib, form, kind, c, 256)[0]["want_part"] == want, (form, c)
    # ... and the example of a partitioned chip: a forced c = 14 at 32 compute units
    if kind == 0 and form == 0:
        plan, launches = rsm.query(lib, 0, 0, 14, 32)
        assert plan["two_len"] == 64 == 1 << plan["lo_bits"] and plan["want_part"] == 1
        assert launches[0]["jobs"][0]["out_buf"] == rsm.ROWCOL and launches[1]["jobs"][0]["groups"] == 0   # Sr = 1


def test_the_matrix_reaches_every_path(lib):
    """Runs after the replays above (and repeats the queries when run alone)."""
    for form in rsm.FORMS:
        facts = set()
        for kind in rsm.KINDS:
            if (form, kind) not in _coverage:
                _coverage[(form, kind)] = {f for c in CS for n in NUM_CUS for f in rsm.coverage(*rsm.query(lib, form, kind, c, n))}
            facts |= _coverage[(form, kind)]
        want = {("worker", k, w) for k, w in rsm.WORKERS[form]}
        want |= {("want_part", False), ("t_from_cols", False), ("t_from_cols", True), ("lo_bits", 0)}
        if form in (0, 1):
            want |= {("want_part", True), ("Sr>1", True), ("Sr>1", False), ("Sc>1", True)}
        # Unreachable, and why:
        #   one-lane G2 (form 2): want_part - the two-stage sums exist for FpOps and Fp2K3Ops alone (TWO_STAGE_FR), so no Sr, Sc;
        #   Sc = 1 (forms 0, 1): Sc = H / min(two_len, H) = 1 needs H <= 64, i.e. at most 2^12 buckets a window (H >= Lw), and
        #     want_part needs NB >= 2^17, i.e. W >= 32 windows - but Lw >= 32 means c >= 11, and ceil(256 / 11) = 24.
        assert want <= facts, (rsm.FORMS[form], sorted(want - facts, key=str))
        assert ("Sc>1", False) not in facts and (form != 2 or ("want_part", True) not in facts), "reachable after all: test it"


def test_the_replay_notices_a_wrong_plan(lib):
    """the model's own checks, on records edited by hand"""
    plan, launches = rsm.query(lib, 0, 0, 14, 256)   # 19 windows of 2^13 buckets, summed in two stages
    assert plan["want_part"] and len(launches) == 3
    buckets = rsm.seeded_buckets(plan, 1)
    rsm.check_plan(plan, launches, buckets)

    def edited(li, q, **kw):
        out = [dict(l, jobs=[dict(j) for j in l["jobs"]]) for l in launches]
        out[li]["jobs"][q].update(kw)
        return out

    last = len(launches) - 1
    for what in (edited(0, 0, out_off=launches[0]["jobs"][0]["out_off"] + 1),      # a cell unwritten, one written twice
                 edited(0, 1, istride=launches[0]["jobs"][1]["stride"], stride=1),   # columns read as rows
                 edited(last, 0, group_shift=launches[last]["jobs"][0]["group_shift"] + 1),
                 edited(last, 2, lanes=3),
                 edited(1, 0, groups=0),                                             # the second stage switched off
                 launches[:1] + launches[2:]):
        with pytest.raises(rsm.PlanError):
            rsm.check_plan(plan, what, buckets)


# ---------------------------------------------------------------------------------------------------------- the host tail
TAIL_CS = (2, 3, 8, 13, 16, 20, 24)
MAX_K = 64


class Records:
    """raw records of k G for |k| <= MAX_K, every one in a scaling and with +p masks of its own"""

    def __init__(self, g):
        self.g, self.rnd = g, random.Random("host tail %d" % g)
        self.pool = gm.subgroup_points(g, MAX_K)
        self.lam = gm._lambda_source(g, "host tail")
        self.nmask = 4 * gm.FIELDS[g].width

    def rec(self, k, garbage=False):
        if k == 0:
            return gm.identity_record(self.g, self.rnd if garbage else None)
        pt = self.pool[abs(k) - 1]
        return gm.represent(self.g, pt if k > 0 else gm.neg(self.g, pt), next(self.lam), self.rnd.randrange(1 << self.nmask))


_records = {}


def tail_cases(plan, rnd):
    """name -> the integer k of every record of bits (the record is k G)"""
    W, c = plan["W"], plan["c"]
    n, cb = W * c, c - 1
    out = {
        "random": [rnd.randrange(-MAX_K, MAX_K + 1) for _ in range(n)],
        "identities": [0] * n,
        "same_point": [3] * n,
        "alternating": [5 if i % 2 == 0 else -5 for i in range(n)],
    }
    # one live record: U[0][0] and U[W-1][c-2] in the layout ([W][lo_bits] low bits, [W][hi_bits] high bits), T[0], T[W-1]
    lo, hi = plan["lo_bits"], plan["hi_bits"]
    u00 = 0 if lo else W * lo                                  # (c = 2: bit 0 is a high bit)
    ulast = W * lo + (W - 1) * hi + (hi - 1)
    for name, at in (("live_U00", u00), ("live_Ulast", ulast), ("live_T0", W * cb), ("live_Tlast", W * cb + W - 1)):
        out[name] = [7 if i == at else 0 for i in range(n)]
    return out


@pytest.mark.parametrize("g", (1, 2), ids=("g1", "g2"))
@pytest.mark.parametrize("kind", sorted(rsm.KINDS), ids=lambda k: rsm.KINDS[k])
@pytest.mark.parametrize("c", TAIL_CS)
def test_host_tail_against_integers(lib, c, kind, g):
    plan = rsm.query(lib, 0 if g == 1 else 2, kind, c, 256)[0]
    recs = _records.setdefault(g, Records(g))
    rnd = random.Random("tail cases %d %d %d" % (c, kind, g))
    abytes = 2 * 48 * gm.FIELDS[g].width
    assert plan["affine"] == abytes
    # the weights the walk must give the live records
    W = plan["W"]
    want_weight = {"live_U00": 1, "live_Ulast": (1 << (c - 2)) << (c * (W - 1)), "live_T0": 1, "live_Tlast": 1 << (c * (W - 1))}
    for name, ks in tail_cases(plan, rnd).items():
        total = rsm.tail(plan, ks)
        if name in want_weight:
            assert total == 7 * want_weight[name], (name, c, kind)
        raw = gm._pack([recs.rec(k, garbage=(i % 3 == 1)) for i, k in enumerate(ks)])
        out = np.full(abytes + 64, 0xA5, dtype=np.uint8)
        assert lib.bh_test_msm_host_tail(g, kind, c, gm._ptr(raw), gm._ptr(out)) == 0
        assert (out[abytes:] == 0xA5).all()
        k = total % bls.Q
        want = gm.mul(g, gm.GEN[g], k) if k else None
        if name == "identities":
            assert want is None
        assert gm._unpack(out[:abytes], 1)[0] == gm.affine_record(g, want), (name, c, rsm.KINDS[kind], g)


def test_hooks_refuse_what_they_document(lib):
    out, n = (ctypes.c_uint32 * 16)(), ctypes.c_size_t()
    for form, kind, c, num_cus in ((3, 0, 8, 256), (-1, 0, 8, 256), (0, 2, 8, 256), (0, 0, 1, 256), (0, 0, 25, 256), (0, 0, 8, -1),
                                   (0, 0, 8, 0)):   # (0 compute units: the context's own, and there is none)
        assert lib.bh_test_reduce_plan(None, form, kind, c, num_cus, out, None, 0, ctypes.byref(n)) != 0, (form, kind, c, num_cus)
    buf = np.zeros(4096, dtype=np.uint8)
    for g, kind, c in ((0, 0, 8), (3, 0, 8), (1, 2, 8), (1, 0, 1), (1, 0, 25)):
        assert lib.bh_test_msm_host_tail(g, kind, c, gm._ptr(buf), gm._ptr(buf)) != 0, (g, kind, c)
    # the device hook refuses before it touches a device (no context here: that alone is refused too)
    assert lib.bh_test_reduce_stage_dev(None, 0, 0, 8, 256, gm._ptr(buf), gm._ptr(buf), gm._ptr(buf), gm._ptr(buf), gm._ptr(buf), gm._ptr(buf)) != 0
