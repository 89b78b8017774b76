"""The one-launch small path and the error-resolution pass without a GPU: the integer model of msm_small_fill_kernel
(tests/models/small_fill_model.py) against brute force, the shipped gate (small_fill_plan of csrc/msm_stage_plans.hpp over
make_table_plan, through the host-only hook bh_test_small_fill_plan) against the model's restatement and against what the
kernel's LDS, 16-bit entry ids and 16-bit digits can hold, a pin of the sizes that take the path today, and
err_resolve_lo_ref against the reference's ceil(ln n) rule."""
import random

import numpy as np
import pytest

from tests.models import small_fill_inputs as inputs
from tests.models import small_fill_model as model
from tests.models import sort_stage_inputs as ssi
from tests.models import sort_stage_model as ssm

# the largest nd that takes the path over dense rows of ceil(256 / c) windows; every nd from 1 up to it does, none beyond
FUSED_UP_TO = {4: 1, 5: 3, 6: 8, 7: 19, 8: 51, 9: 55, 10: 159, 11: 47, 12: 95, 13: 1075, 14: 103, 15: 12}


@pytest.fixture(scope="module")
def lib():
    return ssi.test_lib()


def plan(lib, form, nd, c, row_records=None, flags=0):
    return inputs.plan_info(form, nd, c, row_records, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# the model against brute force
# ---------------------------------------------------------------------------------------------------------------------------
def model_cases():
    out = []
    for c, nd in ((13, 70), (10, 159), (8, 51), (5, 3), (4, 1), (15, 12), (7, 19)):
        for vec in inputs.VECTORS:
            for dens, skip, nb in (("none", 0, "all"), ("random", 5, "last"), ("bit64", 0, "all"), ("ones", 2, "mid_zero")):
                if dens == "bit64" and nd <= 64:
                    continue
                out.append(inputs.case(0, c, nd, vec, 0 if vec == "over_q" else (c + skip) & 1, dens=dens, skip=skip, nb=nb))
    return out


@pytest.mark.parametrize("case", model_cases(), ids=inputs.case_id)
def test_model_against_brute_force(case):
    """over a consistent table t[w][k] = 2^(c w) t_k: sum_d d bucket_d == sum_i s_i t_(k_i) over the integers, every non-zero
    digit of a live scalar is an entry of exactly one list exactly once, and the four sub-workers share a bucket's entries -
    on both routes (the list cap lowered to 0 sends every bucket down the scan)"""
    inp = inputs.build(case)
    c, nd = inp["c"], inp["nd"]
    rng = random.Random(inputs.case_id(case))
    bases = [rng.randrange(1, 1 << 40) for _ in range(inp["row_records"])]
    tab = inputs.consistent_table(c, bases)
    args = (c, inp["raw"], inp["fmt"], inp["density"], inp["skip"], inp["n_bases"])
    want = model.brute_total(*args, bases)
    dense, k, live, eof, _ = ssm.density_rank(nd, inp["density"], inp["skip"], inp["n_bases"])
    values = [v if l else 0 for v, l in zip(ssm.load_scalars(inp["raw"], inp["fmt"]), live)]
    for cap in (model.LIST_CAP, 0):
        m = model.fill(*args, tab, list_cap=cap)
        assert sum(d * b["sum"] for d, b in m["buckets"].items()) == want
        assert m["eof"] == int(eof) and m["ident"] == 0
        assert [int(x) for x in m["kidx"]] == [int(ki) if l else model.NO_KIDX for ki, l in zip(k, live)]
        # the digits say the scalar
        half = 1 << (c - 1)
        for i in range(nd):
            col = [int(d) for d in m["dig"][:, i]]
            assert sum(d << (c * w) for w, d in enumerate(col)) == values[i] and all(-half < d <= half for d in col)
        seen = []
        for d, b in m["buckets"].items():
            assert b["overflow"] == (len(b["entries"]) > cap)
            assert sorted(e for part in b["subs"] for e in part) == b["entries"] and len(b["subs"]) == model.LANES_PER_BUCKET
            assert max(len(p) for p in b["subs"]) - min(len(p) for p in b["subs"]) <= 1
            assert all(abs(int(m["dig"].reshape(-1)[e])) == d for e in b["entries"])
            seen += b["entries"]
        assert sorted(seen) == [int(e) for e in np.flatnonzero(m["dig"].reshape(-1))] and len(seen) == len(set(seen))
    if case["vec"] == "capedge" and nd * ssi.full_windows(c) >= 3 * model.LIST_CAP:
        m = model.fill(*args, tab)
        if case["dens"] == "none":
            sizes = sorted(len(b["entries"]) for b in m["buckets"].values())
            assert sizes == [model.LIST_CAP - 1, model.LIST_CAP, model.LIST_CAP + 1]
            assert [b["overflow"] for b in m["buckets"].values()].count(True) == 1


def test_identity_records_are_flagged_and_skipped():
    inp = inputs.build(inputs.case(0, 8, 51, "random", 0, ident="hit"))
    m = inputs.expected(inp)
    assert m["ident"] == 1
    inp = inputs.build(inputs.case(0, 8, 51, "random", 0, ident="unseen"))
    assert (inp["table"] == 0).any() and inputs.expected(inp)["ident"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------------
def test_shipped_constants_are_the_models(lib):
    p = plan(lib, 0, 9, 13)
    assert (p["MAX_SCALARS"], p["MAX_ENTRIES"], p["MAX_PER_BUCKET"], p["LIST_CAP"], p["LANES_PER_BUCKET"], p["threads"]) == (
        model.MAX_SCALARS, model.MAX_ENTRIES, model.MAX_PER_BUCKET, model.LIST_CAP, model.LANES_PER_BUCKET, model.THREADS)
    assert (p["xyzz"], p["affine"], p["err_bytes"]) == (192, 96, 40) and plan(lib, 3, 9, 13)["xyzz"] == 384 and plan(lib, 1, 9, 13)["affine"] == 192


@pytest.mark.parametrize("form", sorted(model.FORMS), ids=lambda f: model.FORMS[f])
def test_gate_against_the_model_and_the_kernels_limits(lib, form):
    """nd = 1 .. 2100, c = 2 .. 16: the shipped plan equals the restatement, and wherever it fuses the kernel's dynamic LDS fits a
    workgroup, an entry id its list's 16 bits, a digit a short, the density prefix 32 words, a workgroup's buckets its threads,
    and the grid covers every bucket"""
    fused_nd = {}
    for c in range(2, 17):
        for nd in range(1, 2101):
            p = plan(lib, form, nd, c)
            g = model.gate(form, nd, c)
            assert {k: p[k] for k in g} == g, (form, nd, c)
            if p["fused"]:
                fused_nd.setdefault(c, []).append(nd)
                assert p["lds"] <= 64 * 1024
                assert p["entries"] <= 65535 and p["entries"] == p["Wd"] * nd
                assert (1 << (c - 1)) <= 32767 and p["nb"] == 1 << (c - 1)
                assert (nd + 63) // 64 <= 32
                assert 0 < p["bpb"] <= p["threads"] and p["bpb"] * p["LANES_PER_BUCKET"] <= p["threads"]
                assert p["workgroups"] * p["bpb"] >= p["nb"] and (p["workgroups"] - 1) * p["bpb"] < p["nb"]
    # what ships: a change of the gate changes a line of FUSED_UP_TO.  The default 13-bit tables keep every MiMC-sized job
    # (9 .. 1023 terms) on the path; nothing fuses for c <= 3 or c >= 16
    assert {c: nds for c, nds in fused_nd.items()} == {c: list(range(1, top + 1)) for c, top in FUSED_UP_TO.items()}
    assert FUSED_UP_TO[13] >= 1023


def test_gate_flags_rows_and_refusals(lib):
    assert plan(lib, 0, 322, 13)["fused"] == 1 and plan(lib, 0, 322, 13, flags=model.NO_SMALL_PATH)["fused"] == 0
    assert model.gate(0, 322, 13, flags=model.NO_SMALL_PATH)["fused"] == 0
    assert model.gate(0, 322, 13, small_path=False)["fused"] == 0 and model.gate(0, 322, 13, many=True)["fused"] == 0
    # the records per row do not enter the gate
    assert plan(lib, 2, 322, 13, row_records=5000) == plan(lib, 2, 322, 13)
    for bad in ((4, 9, 13, 9), (-1, 9, 13, 9), (0, 0, 13, 9), (0, 9, 1, 9), (0, 9, 25, 9), (0, 9, 13, 0), (0, 9, 13, (1 << 31) // 20 + 1),
                (0, (1 << 32) // 20 + 1, 13, 9)):
        assert plan(lib, *bad) is None, bad


def test_dev_hooks_refuse_without_a_context(lib):
    buf = np.zeros(1 << 12, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.bh_test_small_fill_dev(None, 0, 13, p, 0, 9, None, 0, 9, p, 12, p, None, p, p) != 0
    assert lib.bh_test_err_resolve_dev(None, 1, p, 0, 9, None, None, 0, 9, p, 9, 96, 0, p, p) != 0


# ---------------------------------------------------------------------------------------------------------------------------
# the error-resolution pass
# ---------------------------------------------------------------------------------------------------------------------------
def test_lo_ref_against_the_references_rule(lib):
    """the integer neighbours of e^6, e^7, e^8 (where ceil(ln n) steps), the n < 32 branch, and the far end"""
    want = {0: 252, 1: 252, 31: 252, 32: 252, 33: 252, 403: 252, 404: 252, 1096: 252, 1097: 248, 2980: 248, 2981: 252}
    for nref in (0, 1, 31, 32, 33, 403, 404, 1096, 1097, 2980, 2981, 1 << 20, 1 << 24, (1 << 32) - 1):
        got = lib.bh_test_err_resolve_lo_ref(nref)
        assert got == model.lo_ref(nref), nref
        assert got < 256 and (nref not in want or got == want[nref]), (nref, got)
    # ceil(ln n) itself: 403 < e^6 < 404, 1096 < e^7 < 1097, 2980 < e^8 < 2981
    assert [model.ceil_ln(n) for n in (32, 403, 404, 1096, 1097, 2980, 2981, 1 << 20, (1 << 32) - 1)] == [4, 6, 7, 7, 8, 8, 9, 14, 23]


def test_error_pass_model_on_a_handful():
    Q = ssm.Q
    lo = model.lo_ref(5)
    assert lo == 252
    raw = [(1 << lo) - 1, 1 << lo, Q - 1, 0, Q + (1 << lo) - 1]
    none = [False] * 5
    assert model.err_resolve(raw, 0, None, None, 0, 5, none, 5) == 0
    for k, want in enumerate((0, 1, 1, 0, 0)):     # the over-q value reduces to one below the window
        ident = list(none)
        ident[k] = True
        assert model.err_resolve(raw, 0, None, None, 0, 5, ident, 5) == want, k
    assert model.err_resolve(raw, 0, None, None, 0, 1, [True], 5) == 0            # the scalars with top bits are past the end
    assert model.err_resolve(raw, 0, None, None, 3, 5, [False] * 4 + [True], 5) == 1   # skip = 3: scalar 1 owns base 4
    dens = np.array([0b10110], dtype=np.uint64)    # dense: 1, 2, 4 -> bases 0, 1, 2
    prefix = np.array([0, 3], dtype=np.uint32)
    assert model.err_resolve(raw, 0, dens, prefix, 0, 3, [True, False, False], 5) == 1
    assert model.err_resolve(raw, 0, dens, prefix, 0, 3, [False, False, True], 5) == 0
    assert model.err_resolve(raw, 0, dens, np.array([1, 3], dtype=np.uint32), 0, 3, [False, True, False], 5) == 1   # the prefix is taken as given
