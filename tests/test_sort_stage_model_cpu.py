"""The integer model of the digit and sort stage (tests/models/sort_stage_model.py) and its inputs
(tests/models/sort_stage_inputs.py) against plain Python, and the host-only plan hook bh_test_sort_plan against an independent
restatement of the sizes.  No GPU: what tests/test_gpu_sort_stage.py compares the kernels with is checked here first."""
import ctypes
import random

import numpy as np
import pytest

from tests.models import sort_stage_inputs as inputs
from tests.models import sort_stage_model as model

Q = model.Q
ALL_C = sorted(set(inputs.CLASSIC_C) | set(inputs.TABLE_C))


def ceil_div(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("c", ALL_C)
def test_recoding_sums_back_to_the_scalar(c):
    """sum of +-|d| 2^(c w) = s mod q for every kind of scalar, |d| <= 2^(c-1), no carry out of the top digit, sign clear on 0"""
    rng = random.Random(c)
    kind = inputs.TABLE if c in inputs.TABLE_C else inputs.CLASSIC
    for fmt in (0, 1):
        raws = []
        for vec in inputs.vector_names(kind, c):
            nd = 1100 if vec.startswith("bins") else 40
            raws += inputs.raw_scalars(inputs.values(vec, kind, c, nd, rng), fmt)[:300]
        if fmt == 0:
            raws += inputs.over_q(24, rng)
        vals = model.load_scalars(raws, fmt)
        assert all(v < Q for v in vals)
        if fmt == 0:
            assert all(v == r % Q for v, r in zip(vals, raws))
        else:
            assert all(v * inputs.R % Q == r for v, r in zip(vals, raws))
        mag, sign, carry = model.recode(vals, c)
        assert not carry.any()
        assert int(mag.max()) <= 1 << (c - 1)
        assert not (sign[mag == 0]).any()
        for v, m, s in zip(vals, mag.tolist(), sign.tolist()):
            assert sum((-d if neg else d) << (c * w) for w, (d, neg) in enumerate(zip(m, s))) == v


def test_special_vectors_are_what_their_names_say():
    for c in ALL_C:
        half, W = 1 << (c - 1), model.windows(c)
        full = inputs.full_windows(c)
        mag, sign, _ = model.recode(inputs.values("half", 0, c, 1, None), c)
        assert (mag[0, :full] == half).all() and not sign.any()
        mag, sign, _ = model.recode(inputs.values("halfp1", 0, c, 1, None), c)
        assert sign[0, 0] == 1 and mag[0, 0] == half - 1 and mag[0, full] == 1      # a carry into every row up to the top
        if c > 2:
            assert (sign[0, :full] == 1).all()
        mag, sign, _ = model.recode(inputs.values("carry0", 0, c, 1, None), c)
        assert (mag[0, 1:full] == 0).all() and not sign[0, 1:full].any() and mag[0, full] == 1 and full < W


def python_table_stream(inp, spt):
    """the table plan's stream by Python's sorted over the documented key tuple"""
    c, nd = inp["c"], inp["nd"]
    W = model.windows(c)
    dense, k, live, eof, _ = model.density_rank(nd, inp["density"], inp["skip"], inp["n_bases"])
    vals = model.load_scalars(inp["raw"], inp["fmt"])
    rows = []
    for i in range(nd):
        if not live[i]:
            continue
        carry, s = 0, vals[i]
        for w in range(W):
            v = ((s >> (c * w)) & ((1 << c) - 1)) + carry
            neg = carry = 0
            if v > (1 << (c - 1)):
                v, carry = (1 << c) - v, 1
                neg = 1 if v else 0
            if v:
                rows.append(((v - 1, i // spt, (i % spt) // 64, w, i), (v << 32) | (neg << 31) | ((int(k[i]) + w * inp["stride"]) & 0x7FFFFFFF)))
    return [e for _, e in sorted(rows)], eof


@pytest.mark.parametrize("c", inputs.TABLE_C)
def test_table_stream_equals_pythons_sorted(c):
    for cs in (inputs.case(inputs.TABLE, c, "2*spt+1", "random", c & 1, dens="random", skip=5, nb="minus1"),
               inputs.case(inputs.TABLE, c, "spt+1", "mixed", 1 - (c & 1))):
        inp = inputs.build(cs)
        m = inputs.expected(inp)
        want, eof = python_table_stream(inp, inputs.spt_of(c))
        assert m["stream"].tolist() == want and m["eof"] == int(eof) and m["live"] == len(want)
        assert int(m["zstart"][0]) == model.windows(c) * inp["nd"] - len(want)
        bits = model.table_pass_bits(c)
        assert (m["after"](sum(bits)) == m["stream"]).all()
        # a pass sorts by its key bits alone and is stable
        prev, shift = m["after"](bits[0]), bits[0]
        for b in bits[1:]:
            key = (((prev >> np.uint64(32)).astype(np.int64) - 1) >> shift) & ((1 << b) - 1)
            nxt = m["after"](shift + b)
            assert (prev[np.argsort(key, kind="stable")] == nxt).all()
            prev, shift = nxt, shift + b


@pytest.mark.parametrize("c", inputs.CLASSIC_C)
def test_classic_windows_equal_pythons_stable_sort(c):
    inp = inputs.build(inputs.case(inputs.CLASSIC, c, 203, "mixed", c & 1, dens="random", skip=5, nb="minus1"))
    m = inputs.expected(inp)
    dense, k, live, eof, prefix = model.density_rank(inp["nd"], inp["density"], inp["skip"], inp["n_bases"])
    assert m["eof"] == 1 and eof
    unsorted = m["after"](0)
    assert unsorted.shape == (model.windows(c), inp["nd"])
    # a scalar that is not live contributes digit 0 and still carries its base field
    dead = np.flatnonzero(~live)
    assert len(dead) and (unsorted[:, dead] == (k[dead] & np.uint64(0x7FFFFFFF))[None, :]).all()
    for w in range(model.windows(c)):
        want = sorted(unsorted[w].tolist(), key=lambda e: e >> 32)
        assert m["result"][w].tolist() == want
        assert int(m["zstart"][w]) == sum(1 for e in want if e >> 32 == 0)
    bits = np.unpackbits(inp["density"].view(np.uint8), bitorder="little")
    assert prefix.tolist() == [int(bits[:64 * j].sum()) for j in range(len(inp["density"]))]


def test_every_table_stream_is_what_the_bucket_stage_accepts():
    """stream_ok of csrc/test_bucket_hooks.hip: keys non-decreasing in [1, 2^(c-1)], base fields inside Wd stride"""
    k = inputs.constants()
    seen = 0
    for cs in inputs.all_cases():
        if cs["kind"] != inputs.TABLE:
            continue
        inp = inputs.build(cs)
        m = inputs.expected(inp)
        Wd = model.windows(inp["c"])
        assert Wd * inp["stride"] < 1 << 31 and inp["n_bases"] <= inp["stride"]
        assert model.stream_ok(m["stream"], inp["c"], Wd * inp["stride"]), inputs.case_id(cs)
        assert int(m["zstart"][0]) + m["live"] == Wd * inp["nd"] <= 1 << 21
        if cs["stride"] == "edge":
            # the top row's last records: Wd stride <= 2^31 - 1 < Wd (stride + 1), and k reaches stride - 3
            assert (1 << 31) - 1 - int((m["stream"] & np.uint64(0x7FFFFFFF)).max()) < 8 + Wd
        if cs["vec"].startswith("live:"):
            assert m["live"] == int(eval(cs["vec"][5:], {}, dict(TW=k["TW"])))
        if cs["vec"] == "sparse":
            assert m["live"] < k["TW"]
        if cs["vec"].startswith("bins"):
            shift, bits = inputs.pass_layout(inputs.TABLE, inp["c"])[0][int(cs["vec"][4:])]
            key = (m["stream"] >> np.uint64(32)).astype(np.int64) - 1
            assert len(np.unique((key >> shift) & ((1 << bits) - 1))) == 1 << bits, inputs.case_id(cs)
        seen += 1
    assert seen >= 300


def test_classic_inputs_reach_every_bin_and_fit_the_hook():
    for cs in inputs.all_cases():
        if cs["kind"] != inputs.CLASSIC:
            continue
        nd = inputs.resolve_nd(cs)
        assert model.windows(cs["c"]) * nd <= 1 << 21
        if cs["vec"].startswith("bins"):
            inp = inputs.build(cs)
            m = inputs.expected(inp)
            p = int(cs["vec"][4:])
            d = (m["result"] >> np.uint64(32)).astype(np.int64)
            reachable = min(256, ((1 << (cs["c"] - 1)) >> (8 * p)) + 1)
            assert len(np.unique((d >> (8 * p)) & 255)) >= reachable, inputs.case_id(cs)


def independent_plan(kind, n, c, k):
    """pass count, pass widths, tile counts and the size of the counts array, restated"""
    W = ceil_div(256, c)
    if kind == inputs.CLASSIC:
        tiles = ceil_div(n, k["T"])
        passes = ceil_div(c, 8)
        return dict(n=n, c=c, W=W, nd=n, Wd=W, num_tiles=tiles, sort_passes=passes, base_stride=0, widths=[8] * passes, spt=0, first_tiles=0,
                    counts=W * 256 * tiles)
    widths = model.table_pass_bits(c)
    spt = max(1, min(k["WIDE_THREADS"], k["TW"] // W))
    tiles, first = ceil_div(W * n, k["TW"]), ceil_div(n, spt)
    counts = max([(1 << widths[0]) * first] + [(1 << b) * tiles for b in widths[1:]])
    return dict(n=W * n, c=c, W=1, nd=n, Wd=W, num_tiles=tiles, sort_passes=len(widths), widths=widths, spt=spt, first_tiles=first, counts=counts)


def own_scan_tmp_elems(n, tile):
    tot = 0
    while n > 1:
        n = ceil_div(n, tile)
        tot += (n + 63) & ~63
        if n == 1:
            break
    return tot + 64


def test_plan_hook_agrees_with_an_independent_restatement():
    k = inputs.constants()
    assert (k["T"], k["TW"], k["WIDE_THREADS"], k["SCAN_TILE"], k["guard"], k["sentinel"], k["err_bytes"]) == (4096, 7168, 512, 2048, 4096, 0xA5, 40)
    for c in range(2, 25):
        assert sum(model.table_pass_bits(c)) == c - 1 and max(model.table_pass_bits(c)) <= 10
        assert len(model.table_pass_bits(c)) == ceil_div(c - 1, 10)
    for c, widths in inputs.TABLE_WIDTHS.items():
        assert model.table_pass_bits(c) == widths
    rng = random.Random(1)
    for kind in (inputs.CLASSIC, inputs.TABLE):
        for c in range(2, 25):
            W = ceil_div(256, c)
            sizes = [1, 63, 64, 65, 4095, 4096, 4097, 8193, 1 << 20, (1 << 21) // W, 1 << 21] + [rng.randrange(1, 1 << 22) for _ in range(20)]
            for n in sizes:
                stride = 0 if kind == inputs.CLASSIC else n + 3
                p = inputs.plan_info(kind, n, c, stride)
                want = independent_plan(kind, n, c, k)
                widths = [p["bits%d" % j] for j in range(4)]
                assert widths == want["widths"] + [0] * (4 - len(want["widths"])), (kind, n, c)
                for f in ("n", "c", "W", "nd", "Wd", "num_tiles", "sort_passes", "spt", "first_tiles", "counts"):
                    assert p[f] == want[f], (kind, n, c, f, p[f], want[f])
                assert p["base_stride"] == stride
                assert p["scan_tmp"] == own_scan_tmp_elems(p["counts"] + 1, k["SCAN_TILE"])
    # the plan does not depend on the group or the chip as far as this stage goes
    a, b = inputs.plan_info(inputs.TABLE, 5000, 13, 5000, g2=1, num_cus=64), inputs.plan_info(inputs.TABLE, 5000, 13, 5000)
    assert a == b
    # refused: what msm_enqueue refuses
    assert inputs.plan_info(inputs.TABLE, 0, 13) is None and inputs.plan_info(inputs.TABLE, 5, 1) is None and inputs.plan_info(inputs.TABLE, 5, 25) is None
    assert inputs.plan_info(inputs.CLASSIC, 5, 13, 7) is None
    assert inputs.plan_info(inputs.TABLE, 5, 13, (1 << 31) // 20 + 1) is None and inputs.plan_info(inputs.TABLE, 5, 13, (1 << 31) // 20) is not None
    assert inputs.plan_info(inputs.TABLE, ceil_div(1 << 32, 20), 13) is None


def test_pinned_sizes():
    """literal sizes, so that a sizing function cannot shrink silently; and the case tables, so that they cannot either"""
    # the first pass of a 20-bit table over 2^21 scalars: 1024 bins x 4096 tiles + the total slot = SCAN_TILE^2 + 1 counts
    p = inputs.plan_info(inputs.TABLE, 1 << 21, 20, 1 << 21)
    assert (p["spt"], p["first_tiles"], p["bits0"], p["bits1"], p["counts"]) == (512, 4096, 10, 9, 1 << 22)
    assert p["counts"] + 1 == inputs.scan_sizes()[-1] == 2048 * 2048 + 1
    assert p["scan_tmp"] == 2112 + 64 + 64 + 64
    p = inputs.plan_info(inputs.TABLE, 1 << 20, 13, 1 << 20)
    assert (p["Wd"], p["spt"], p["first_tiles"], p["num_tiles"], p["counts"], p["scan_tmp"]) == (20, 358, 2929, 2926, 187456, 256)
    p = inputs.plan_info(inputs.CLASSIC, 1 << 20, 16)
    assert (p["W"], p["num_tiles"], p["counts"], p["scan_tmp"]) == (16, 256, 1 << 20, 576 + 64 + 64)
    p = inputs.plan_info(inputs.CLASSIC, 8193, 2)
    assert (p["W"], p["num_tiles"], p["counts"], p["scan_tmp"]) == (128, 3, 98304, 192)
    assert inputs.CLASSIC_C == (2, 8, 9, 13, 16, 17, 20, 24) and inputs.TABLE_C == (2, 5, 10, 11, 12, 13, 16, 20, 21, 22, 24)
    assert len(inputs.VECTORS) == 9 and len(inputs.DENSITIES) == 8
    assert len(inputs.scan_sizes()) == 9
    assert (len(inputs.shape_cases()), len(inputs.table_cases()), len(inputs.density_cases())) == PINNED_CASE_COUNTS


PINNED_CASE_COUNTS = (597, 77, 160)


def test_scan_scratch_accesses_stay_inside_the_shipped_size():
    """one slot per tile at each level, the next level starting at the count rounded up to 64"""
    lib = inputs.test_lib()
    tile = inputs.constants()["SCAN_TILE"]
    rng = random.Random(2)
    sizes = list(inputs.scan_sizes()) + [tile ** 2 + tile, 1 << 26] + [rng.randrange(1, (1 << 26) + 1) for _ in range(10000)]
    elems = ctypes.c_size_t(0)
    for n in sizes:
        assert lib.bh_test_scan_dev(None, None, n, ctypes.addressof(elems), None, None) == 0
        top, levels = model.scan_layout(n, tile)
        assert top <= elems.value == own_scan_tmp_elems(n, tile), (n, top, elems.value)
        assert levels[-1][1] == 1 and all(off % 64 == 0 for off, _ in levels)
        # levels do not overlap
        for (o0, s0), (o1, _) in zip(levels, levels[1:]):
            assert o0 + s0 <= o1
    assert len(model.scan_layout(tile * tile, tile)[1]) == 2 and len(model.scan_layout(tile * tile + 1, tile)[1]) == 3


def test_scan_model_on_small_data():
    data = np.array([3, 0, 5, 1, 1, 7, 2], dtype=np.uint32)
    assert model.exclusive_scan(data).tolist() == [0, 3, 3, 8, 9, 10, 17]
    tmp = model.scan_scratch(data, 2, 64 + 64 + 64 + 64, 0xA5A5A5A5)
    # tiles of 2: sums 3 6 8 2 -> scanned 0 3 9 17; next level sums 9 10 -> 0 9; last level: the total
    assert tmp[:4].tolist() == [0, 3, 9, 17] and tmp[64:66].tolist() == [0, 9] and tmp[128] == 19
    assert (np.delete(tmp, [0, 1, 2, 3, 64, 65, 128]) == 0xA5A5A5A5).all()
