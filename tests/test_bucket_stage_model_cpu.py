"""The index model of stage 4 (tests/models/bucket_stage_model.py) against brute force, the shipped queue bounds
(merge_bounds of csrc/msm_stage_plans.hpp through bh_test_merge_plan) against the model's counts, and the shipped merge_plan against
the formulas msm_enqueue computed inline before they moved.  No GPU: bh_test_merge_plan and bh_test_bucket_stage_shape are
host code."""
import ctypes
import math

import pytest

from tests.models import bucket_stage_model as model
from tests.models import bucket_stage_streams as streams

MERGE_FORMS = range(6)
SMALL_SET = {5}                  # the form that runs only on sets of at most 128 buckets
ACC_OF = {0: 0, 1: 0, 2: 4, 3: 4, 4: 2, 5: 2}
RAW = {"g1": 6, "k3": 7, "g2": 8}


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load().test


def shape(lib, merge_form):
    out = (ctypes.c_size_t * 12)()
    assert lib.bh_test_bucket_stage_shape(ACC_OF[merge_form], merge_form, out) == 0
    return [int(v) for v in out]


def merge_plan(lib, form, W, n, c, K, cpw, overrides=None, num_cus=256):
    out = (ctypes.c_uint32 * 8)()
    ov = (ctypes.c_uint32 * 4)(*overrides) if overrides else None
    assert lib.bh_test_merge_plan(form, W, n, c, K, cpw, num_cus, ov, out) == 0, (form, W, n, c, K, cpw, overrides)
    return dict(zip(("walk", "run_lanes", "runs_on_pairs", "big_chunks", "piece", "max_long", "max_big", "max_pieces"), map(int, out)))


def run_model(s, plan):
    return model.stage(s["windows"], s["zstart"], s["scalars"], s["K"], s["chunks_per_window"], plan["walk"], plan["big_chunks"],
                       plan["piece"])


def form_streams(lib):
    for form in MERGE_FORMS:
        piece = shape(lib, form)[2]
        for name in streams.STREAM_NAMES:
            s = streams.stream(name, piece, form in SMALL_SET)
            yield form, s, merge_plan(lib, form, s["W"], s["n"], s["c"], s["K"], s["chunks_per_window"], s["overrides"])


# ------------------------------------------------------------------------------------------------------ model self-checks
def test_model_against_brute_force_and_its_own_invariants(lib):
    seen = set()
    for form, s, plan in form_streams(lib):
        key = (s["name"], plan["piece"], s["c"], plan["walk"], plan["big_chunks"])
        if key in seen:
            continue
        seen.add(key)
        m = run_model(s, plan)
        for w, win in enumerate(m["windows"]):
            entries, z, n, tag = s["windows"][w], s["zstart"][w], s["n"], (s["name"], plan["piece"], w)
            assert win["buckets"] == model.brute_buckets(entries, z, s["scalars"]), tag
            # every live entry lies in exactly one partial
            cover = [0] * n
            for lane, d, dest, acc, begin, end in win["partials"]:
                assert begin < end and all(e[0] == d for e in entries[begin:end]), tag
                for p in range(begin, end):
                    cover[p] += 1
            assert cover == [0] * z + [1] * (n - z), tag
            # every partial has exactly one destination (window() refuses two stores to one place), of the right kind
            for lane, d, (kind, index), acc, begin, end in win["partials"]:
                assert kind in ("bucket", "head", "tail") and index == (d if kind == "bucket" else lane), tag
            # every run takes exactly one route, and the runs consume every head and every tail partial exactly once
            owners = [r[0] for r in win["runs"]]
            assert len(set(owners)) == len(owners) and all(r[3] in ("owner", "medium", "big") for r in win["runs"]), tag
            heads = [j for lane, d, last, route, np_ in win["runs"] for j in range(lane + 1, last + 1)]
            assert sorted(heads) == sorted(win["head"]) and sorted(owners) == sorted(win["tail"]), tag
            for lane, d, last, route, np_ in win["runs"]:
                L = last - lane
                assert route == ("big" if L > plan["big_chunks"] else "medium" if L > plan["walk"] else "owner"), tag
                assert np_ == (math.ceil((L + 1) / plan["piece"]) if route == "big" else 0), tag
    assert len(seen) >= 3 * len(streams.STREAM_NAMES)


def test_placed_streams_hold_the_lengths_they_are_built_for(lib):
    """boundaries / branches: every L the issue names, in both windows; loops: the counts its grid-stride loops need"""
    for form in MERGE_FORMS:
        sh = shape(lib, form)
        piece = sh[2]
        for name in ("boundaries", "branches"):
            s = streams.stream(name, piece, form in SMALL_SET)
            plan = merge_plan(lib, form, s["W"], s["n"], s["c"], s["K"], s["chunks_per_window"], s["overrides"])
            assert (plan["walk"], plan["big_chunks"], plan["piece"]) == (streams.WALK, streams.BIG, piece)
            m = run_model(s, plan)
            assert s["n"] % s["K"] and len(set(s["zstart"])) == 2 and s["windows"][0][s["zstart"][0]:] != s["windows"][1][s["zstart"][1]:]
            got = [sorted(r[2] - r[0] for r in win["runs"] if win["views"][r[0]][0] % s["K"] != 0) for win in m["windows"]]
            small = [1, 2, plan["walk"], plan["walk"] + 1, plan["walk"] + 2, plan["big_chunks"], plan["big_chunks"] + 1]
            assert got[0] == sorted(small + [piece - 1, 2 * piece]), (form, name, got[0])
            assert got[1] == sorted(small[:6] + [plan["big_chunks"] + 1, piece, 2 * piece - 1]), (form, name, got[1])
            for w, win in enumerate(m["windows"]):
                z, n, K = s["zstart"][w], s["n"], s["K"]
                for lane, d, last, route, np_ in win["runs"]:
                    first = next(p for p in range(z, n) if s["windows"][w][p][0] == d)
                    assert (first - z) % K == K - 1, "a run starts at the last entry of a chunk"
                assert s["windows"][w][n - 1][0] == win["runs"][-1][1], "the last run ends at the last entry"
                assert all(e[0] == s["windows"][w][z][0] for e in s["windows"][w][:z]), "garbage with the first live digit"
            assert {r for win in m["windows"] for r in (x[3] for x in win["runs"])} == {"owner", "medium", "big"}
            assert m["ident"] == (1 if name == "branches" else 0)
        s = streams.stream("loops", piece, form in SMALL_SET)
        plan = merge_plan(lib, form, s["W"], s["n"], s["c"], s["K"], s["chunks_per_window"], s["overrides"])
        m = run_model(s, plan)
        per_round = 4 * sh[3] // sh[5]          # four wavefronts, G at its smallest
        assert m["nlong"] > per_round and all(m["nlong"] % (sh[3] // G) for G in (8, 16, 32, 64) if G <= sh[3] and sh[3] // G > 1)
        assert m["nbig"] >= 5 and m["npieces"] >= 7 and s["overrides"][3] == 1
        s = streams.stream("effective-K32", piece, form in SMALL_SET)
        Ks = [model.effective_chunk(s["n"], z, s["chunks_per_window"], s["K"]) for z in s["zstart"]]
        assert 8 < Ks[0] < 32 and Ks[1] == 8 and (s["n"] - s["zstart"][1] + 7) // 8 < s["chunks_per_window"] and s["zstart"][2] == s["n"]
        s = streams.stream("effective-K4", piece, form in SMALL_SET)
        assert [model.effective_chunk(s["n"], z, s["chunks_per_window"], s["K"]) for z in s["zstart"]] == [4, 4]


# ------------------------------------------------------------------------------------------------------------ the bounds
def check_bounds(m, plan, tag):
    assert m["nlong"] <= plan["max_long"], (tag, m["nlong"], plan)
    assert m["nbig"] <= plan["max_big"], (tag, m["nbig"], plan)
    assert m["npieces"] <= plan["max_pieces"], (tag, m["npieces"], plan)


def test_shipped_bounds_hold_on_the_gpu_streams(lib):
    for form, s, plan in form_streams(lib):
        check_bounds(run_model(s, plan), plan, (form, s["name"]))


@pytest.mark.parametrize("form", MERGE_FORMS)
def test_shipped_bounds_hold_on_adversarial_streams(lib, form):
    """the shortest medium runs (walk + 2 chunks) and the shortest big runs (big_chunks + 2 chunks) packed back to back, one run
    over the whole window; then the same behind a large z under a plan K of 32, where the effective chunk is 8"""
    small = form in SMALL_SET
    c = 7 if small else 9
    nchunks = 40 if small else 150          # 2 (nchunks / L) + 1 buckets fit the set
    for big_z in (False, True):
        K = 32 if big_z else 8
        for kind in ("medium", "big", "one"):
            probe = merge_plan(lib, form, 1, nchunks * 8, c, K, nchunks)
            L = probe["walk"] + 1 if kind == "medium" else probe["big_chunks"] + 1
            chunks = nchunks if kind != "big" else max(nchunks, 3 * (L + 1))
            live = streams.one_run(8, chunks) if kind == "one" else streams.packed(8, L, chunks)
            assert len(live) <= chunks * 8
            if big_z:
                cpw = (len(live) + 7) // 8
                n = 32 * cpw
                z = n - len(live)
                assert model.effective_chunk(n, z, cpw, K) == 8
            else:
                cpw, n, z = (len(live) + 7) // 8, len(live), 0
            entries = [(live[0][0], 0, 1)] * z + live
            plan = merge_plan(lib, form, 1, n, c, K, cpw)
            m = model.stage([entries], [z], streams.POOL, K, cpw, plan["walk"], plan["big_chunks"], plan["piece"])
            check_bounds(m, plan, (form, kind, big_z))
            if kind == "medium":
                assert m["nlong"] >= (chunks - 2) // L and m["nbig"] == 0, (form, big_z, m["nlong"])
            elif kind == "big":
                assert m["nbig"] >= 2 and m["nlong"] == 0, (form, big_z)
            else:
                assert (m["nlong"], m["nbig"]) == (0, 1) and m["npieces"] == -(-chunks // plan["piece"]), (form, big_z)


def test_plan_query_refuses_what_a_launch_could_not_take(lib):
    out = (ctypes.c_uint32 * 8)()

    def rc(form, W, n, c, K, cpw, ov=None):
        return lib.bh_test_merge_plan(form, W, n, c, K, cpw, 256, (ctypes.c_uint32 * 4)(*ov) if ov else None, out)

    assert rc(0, 2, 1000, 9, 8, 125) == 0
    assert rc(0, 2, 1001, 9, 8, 125) != 0          # n > chunks_per_window K
    assert rc(0, 2, 1000, 9, 8, 125, [0, 12, 0, 0]) != 0 and rc(0, 2, 1000, 9, 8, 125, [0, 4, 0, 0]) != 0      # G: a power of two from 8
    assert rc(1, 2, 1000, 9, 8, 125, [0, 64, 0, 0]) != 0 and rc(0, 2, 1000, 9, 8, 125, [0, 64, 0, 0]) == 0     # ... that fits the worker
    assert rc(4, 2, 1000, 7, 8, 125) != 0 and rc(5, 2, 1000, 7, 8, 125) == 0 and rc(5, 2, 1000, 9, 8, 125) != 0  # fused / split by NB
    assert rc(0, 2, 1000, 9, 8, 125, [40, 0, 32, 0]) != 0                                                       # big_chunks < walk
    assert rc(9, 2, 1000, 9, 8, 125) != 0 and rc(0, 0, 1000, 9, 8, 125) != 0 and rc(0, 2, 1000, 1, 8, 125) != 0


# -------------------------------------------------------------------------------------------------- merge_plan as before
def parent_merge_plan(bundle, n, nb, NB, chunk, nslots, num_cus):
    """what msm_enqueue computed inline before merge_plan existed, restated from that code"""
    full_pw = {"g1": 64, "k3": 16, "g2": 64}[bundle]
    half_pw = {"g1": 32, "k3": 8, "g2": None}[bundle]
    level_us, half_level_us = (37.0, 20.0) if bundle == "k3" else (19.0, 10.5)
    walk = 4
    avg_chunks = float(n) / float(nb) / float(chunk)
    best = [1e30, 8, False]

    def sweep(per_wave, us, pairs):
        g, lg = 8, 3
        while g <= per_wave:
            steps = math.ceil(max(1.0, avg_chunks) / g) + lg
            waves = float(NB) * g / float(per_wave)
            cost = steps * us * max(1.0, waves / (float(num_cus) * 4))
            if cost < best[0]:
                best[:] = [cost, g, pairs]
            g, lg = g << 1, lg + 1

    sweep(full_pw, level_us, False)
    if half_pw:
        sweep(half_pw, half_level_us, True)
        if avg_chunks <= 1.0:
            best[1:] = [8, True]
    run_lanes, pairs = best[1], best[2]
    big_chunks = max(max(32, 4 * run_lanes), int(2.0 * float(n) / float(nb) / float(chunk)))
    piece = 2 * 4 * (half_pw or full_pw)
    max_long = nslots // (walk + 1) + 1
    max_big = nslots // (big_chunks + 1) + 1
    max_pieces = (nslots + max_big) // piece + max_big + 1
    return dict(walk=walk, run_lanes=run_lanes, runs_on_pairs=int(pairs), big_chunks=big_chunks, piece=piece, max_long=max_long,
                max_big=max_big, max_pieces=max_pieces)


def ilog2(v):
    return v.bit_length() - 1


def table_plan_fields(nd, g2, num_cus):
    """(W, n, c, K, chunks_per_window) of make_table_plan over a table of table_window_bits rows (csrc/msm_stages.hip), restated:
    the product library exports no query for it"""
    lg = ilog2(nd)
    if g2:
        c = 13 if lg <= 10 else 8 if lg == 11 else 10 if lg <= 13 else 16
    else:
        c = 13 if lg <= 10 else 10 if lg <= 14 else 13 if lg <= 18 else 20 if lg <= 24 else 24
    Wd = (256 + c - 1) // c
    n = Wd * nd
    lgn = ilog2(n)
    base_k = 8 if lgn <= 20 else 16 if lgn <= 22 else 64 if g2 else 32
    avg = n >> (c - 1)
    lanes_min = num_cus * 4 * 64 * (1 if g2 else 2)
    k = max(base_k, avg)
    k = min(k, max(base_k, n // lanes_min))
    if not g2 and n // lanes_min > k:
        per = (n + lanes_min - 1) // lanes_min
        rounds = max(2, (per + 127) // 128)
        k = max(k, (n + lanes_min * rounds - 1) // (lanes_min * rounds))
    if g2 and c >= 18:
        workers = num_cus * 4 * 2 * 32
        per = (n + workers - 1) // workers
        rounds = max(2, (per + 63) // 64)
        k = max(8, (n + workers * rounds - 1) // (workers * rounds))
    return 1, n, c, k, (n + k - 1) // k


SIZES = [(1 << k) + 17 * k for k in (8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22)]


@pytest.mark.parametrize("bundle", ["g1", "k3", "g2"])
def test_merge_plan_computes_what_msm_enqueue_computed_inline(lib, bundle):
    from bellman_amd import _lib

    product = _lib.load().product
    g2 = bundle != "g1"
    checked = 0
    for num_cus in (256, 64):
        for nd in SIZES:
            out = (ctypes.c_uint * 9)()
            assert product.bh_msm_plan_info(nd, 2 if g2 else 1, 0, out) == 0
            c, W, nb, K, cpw = (int(v) for v in out[:5])
            assert nb == 1 << (c - 1)
            for fields in ((W, nd, c, K, cpw), table_plan_fields(nd, g2, num_cus)):
                W_, n_, c_, K_, cpw_ = fields
                want = parent_merge_plan(bundle, n_, 1 << (c_ - 1), W_ << (c_ - 1), K_, W_ * cpw_, num_cus)
                assert merge_plan(lib, RAW[bundle], W_, n_, c_, K_, cpw_, None, num_cus) == want, (bundle, num_cus, fields)
                checked += 1
    assert checked == 2 * 2 * len(SIZES)
