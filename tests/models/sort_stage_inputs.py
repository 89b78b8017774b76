"""Inputs of the digit and sort stage tests (tests/test_gpu_sort_stage.py, tests/test_sort_stage_model_cpu.py): the smallest
shapes that reach each tile, key and word edge.  The tile sizes come from bh_test_sort_plan (plan_info), never from here.

A case is a small dict (cheap to list at collection time); build(case) turns it into the arrays a run needs."""
import random

import numpy as np

from tests.models import sort_stage_model as model

Q = model.Q
R = (1 << 256) % Q
CLASSIC, TABLE = 0, 1
PLAN_FIELDS = ("n", "c", "W", "nd", "Wd", "num_tiles", "sort_passes", "base_stride", "bits0", "bits1", "bits2", "bits3", "spt",
               "first_tiles", "counts", "scan_tmp", "SORT_TILE", "WIDE_TILE", "WIDE_THREADS", "SCAN_TILE", "guard", "sentinel", "err_bytes")
NUM_CUS = 256

CLASSIC_C = (2, 8, 9, 13, 16, 17, 20, 24)
TABLE_C = (2, 5, 10, 11, 12, 13, 16, 20, 21, 22, 24)
# what table_pass_bits has to give for them (the issue's list): pinned in the CPU test
TABLE_WIDTHS = {2: [1], 5: [4], 10: [9], 11: [10], 12: [6, 5], 13: [6, 6], 16: [8, 7], 20: [10, 9], 21: [10, 10], 22: [7, 7, 7], 24: [8, 8, 7]}
VECTORS = ("random", "zero", "one", "qm1", "half", "halfp1", "carry0", "wave_bins", "mixed")
DENSITIES = ("ones", "zeros", "bit0", "bit63", "bit64", "bit127", "bitlast", "random")

_lib = None


def test_lib():
    global _lib
    if _lib is None:
        from bellman_amd import _lib as loader

        _lib = loader.load().test
    return _lib


_plans = {}


def plan_info(kind, n, c, stride=0, g2=0, num_cus=NUM_CUS):
    """the shipped plan, as a dict of PLAN_FIELDS; None when the hook refuses the arguments"""
    key = (kind, n, c, stride, g2, num_cus)
    if key not in _plans:
        out = np.zeros(len(PLAN_FIELDS), dtype=np.uint64)
        rc = test_lib().bh_test_sort_plan(kind, n, c, stride, g2, num_cus, out.ctypes.data)
        _plans[key] = dict(zip(PLAN_FIELDS, (int(v) for v in out))) if rc == 0 else None
    return _plans[key]


def constants():
    p = plan_info(TABLE, 1, 13)
    return dict(T=p["SORT_TILE"], TW=p["WIDE_TILE"], SCAN_TILE=p["SCAN_TILE"], WIDE_THREADS=p["WIDE_THREADS"], guard=p["guard"],
                sentinel=p["sentinel"], err_bytes=p["err_bytes"])


def spt_of(c):
    return plan_info(TABLE, 1, c)["spt"]


def pass_layout(kind, c):
    """[(shift, bits)] of the key the passes sort by, and what is added to a key to give |d|"""
    if kind == CLASSIC:
        return [(8 * p, 8) for p in range((c + 7) // 8)], 0
    p = plan_info(TABLE, 1, c)
    out, shift = [], 0
    for k in range(p["sort_passes"]):
        out.append((shift, p["bits%d" % k]))
        shift += p["bits%d" % k]
    return out, 1


# ---------------------------------------------------------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------------------------------------------------------
def full_windows(c):
    """windows that lie wholly below bit 254: a value made of digits in them alone is below q"""
    return 254 // c


def pattern(c, first, rest):
    """raw digit `first` in window 0 and `rest` in every other full window"""
    return first + sum(rest << (c * w) for w in range(1, full_windows(c)))


def values(vec, kind, c, nd, rng):
    """nd reduced scalar values"""
    half = 1 << (c - 1)
    if vec == "random":
        return [rng.randrange(Q) for _ in range(nd)]
    if vec == "zero":
        return [0] * nd
    if vec == "one":
        return [1] * nd
    if vec == "qm1":
        return [Q - 1] * nd
    if vec == "half":       # every digit exactly 2^(c-1): the largest key, the all-ones bin of every pass
        return [pattern(c, half, half)] * nd
    if vec == "halfp1":     # every raw digit 2^(c-1) + 1: negative digits, a carry into every row up to the top
        return [pattern(c, half + 1, half + 1)] * nd
    if vec == "carry0":     # raw digits 2^c - 1 that meet a carry: digit 0 with a carry out, sign clear
        return [pattern(c, half + 1, (1 << c) - 1)] * nd
    if vec == "wave_bins":  # a wavefront's 64 entries in one bin next to a wavefront with 64 distinct bins
        out = [rng.randrange(Q) for _ in range(nd)]
        for i in range(min(nd, 64)):
            out[i] = min(5, half)
        for i in range(64, min(nd, 128)):
            out[i] = 1 + (i - 64) % half
        return out
    if vec == "mixed":
        special = [0, 1, Q - 1, pattern(c, half, half), pattern(c, half + 1, half + 1), pattern(c, half + 1, (1 << c) - 1), half, half + 1,
                   (1 << c) - 1, 1 << c]
        return [special[i % 16] if i % 16 < len(special) else rng.randrange(Q) for i in range(nd)]
    if vec.startswith("bins"):   # at least one entry in every bin of pass p
        layout, offset = pass_layout(kind, c)
        shift, bits = layout[int(vec[4:])]
        out = []
        for b in range(1 << bits):
            d = ((b << shift) | rng.getrandbits(shift)) + offset if shift else b + offset
            if d <= half:
                out.append(d << (c * (b % 3)))
        out.append(half)             # the last bin a digit reaches
        assert len(out) <= nd, (vec, c, nd, len(out))
        return out + [rng.randrange(Q) for _ in range(nd - len(out))]
    raise ValueError(vec)


def raw_scalars(vals, fmt):
    return [v * R % Q for v in vals] if fmt == 1 else list(vals)


def over_q(nd, rng):
    """canonical only: raw values in [q, 2^256)"""
    special = [Q, 2 * Q - 1, 2 * Q, (1 << 256) - 1, Q + 1, 2 * Q + 1]
    return [special[i % 8] if i % 8 < len(special) else rng.randrange(Q, 1 << 256) for i in range(nd)]


def live_count_vector(c, target, rng):
    """scalar values whose non-zero digits number exactly `target`, zero scalars among them"""
    W = model.windows(c)
    vals = [rng.randrange(Q) for _ in range(target // max(1, W // 2) + 8)]
    mag, _, _ = model.recode(vals, c)
    cum = np.cumsum((mag != 0).sum(axis=1))
    take = int(np.searchsorted(cum, target, side="right"))
    got = int(cum[take - 1]) if take else 0
    out = vals[:take] + [1] * (target - got) + [0] * 17
    rng.shuffle(out)
    return out


def sparse_tiles_vector(c, rng):
    """four first-pass tiles and a bit, a couple of live scalars in each: the later passes skip whole tiles"""
    spt = spt_of(c)
    nd = 4 * spt + 3
    out = [0] * nd
    for i in range(0, nd, max(1, spt // 2)):
        out[i] = rng.randrange(Q)
    return out


def density_words(dens, nd, rng):
    nwords = (nd + 63) // 64
    bits = np.zeros(nwords * 64, dtype=np.uint8)
    if dens == "ones":
        bits[:nd] = 1
    elif dens == "random":
        bits[:nd] = [rng.getrandbits(1) for _ in range(nd)]
    elif dens == "bitlast":
        bits[nd - 1] = 1
    elif dens.startswith("bit"):
        bits[int(dens[3:])] = 1
    else:
        assert dens == "zeros"
    assert not bits[nd:].any()
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def case(kind, c, nd, vec, fmt, dens="none", skip=0, nb="all", stride="rows", tag=""):
    return dict(kind=kind, c=c, nd=nd, vec=vec, fmt=fmt, dens=dens, skip=skip, nb=nb, stride=stride, tag=tag)


def case_id(cs):
    parts = ["table" if cs["kind"] else "classic", "c%d" % cs["c"], "n%s" % cs["nd"], cs["vec"], "mont" if cs["fmt"] else "canon"]
    if cs["dens"] != "none" or cs["skip"] or cs["nb"] != "all":
        parts += [cs["dens"], "skip%d" % cs["skip"], "nb-" + cs["nb"]]
    if cs["stride"] != "rows":
        parts.append("stride-" + cs["stride"])
    return "-".join(parts + ([cs["tag"]] if cs["tag"] else []))


def resolve_nd(cs):
    """sizes given by name: relative to a tile"""
    nd = cs["nd"]
    if isinstance(nd, int):
        return nd
    k = constants()
    env = dict(T=k["T"], TW=k["TW"], spt=spt_of(cs["c"]) if cs["kind"] else 0)
    return int(eval(nd, {}, env))


def vector_names(kind, c):
    layout, _ = pass_layout(kind, c)
    return VECTORS + tuple("bins%d" % p for p in range(len(layout)))


def shape_cases():
    """every (plan, c, size) with the vectors taking turns, then every vector in both formats at one small size per (plan, c)"""
    out = []
    sizes = {CLASSIC: (1, 63, 64, 65, 255, 256, 257, "T-1", "T", "T+1", "2*T+1"), TABLE: (1, "spt-1", "spt", "spt+1", "2*spt+1")}
    for kind, cs in ((CLASSIC, CLASSIC_C), (TABLE, TABLE_C)):
        for c in cs:
            for j, nd in enumerate(sizes[kind]):
                vec = VECTORS[(j + c) % len(VECTORS)]
                out.append(case(kind, c, nd, vec, (j + c) & 1))
            # more than one tile's worth of entries in a single bin
            out.append(case(kind, c, "2*T+1" if kind == CLASSIC else "2*spt+1", "half", 0, tag="onebin"))
            for vec in vector_names(kind, c):
                for fmt in (0, 1):
                    small = 257 if kind == CLASSIC else "max(spt+1,1030)" if vec.startswith("bins") else "spt+1"
                    out.append(case(kind, c, small, vec, fmt))
            out.append(case(kind, c, 257 if kind == CLASSIC else "spt+1", "over_q", 0))
    return out


def table_cases():
    out = []
    for c in TABLE_C:
        for target in ("TW-1", "TW", "TW+1", "2*TW"):
            out.append(case(TABLE, c, "live", "live:" + target, (c + len(target)) & 1))
        out.append(case(TABLE, c, "sparse", "sparse", c & 1))
        out.append(case(TABLE, c, "spt+1", "random", c & 1, skip=3, stride="small"))
        out.append(case(TABLE, c, "spt+1", "random", 1 - (c & 1), stride="edge"))
    return out


def density_cases():
    out = []
    for kind, c in ((CLASSIC, 13), (TABLE, 13), (TABLE, 22)):
        nd = 203 if kind == CLASSIC else "spt+11"   # neither a multiple of 64
        for dens in DENSITIES:
            for skip in (0, 5):
                for nb in ("all", "minus1", "minus1zero", "none"):
                    if dens == "zeros" and nb != "all":
                        continue   # nothing dense: nothing to drop
                    if nb == "minus1zero" and (skip or dens not in ("ones", "random", "bitlast")):
                        continue   # once per plan and a few maps
                    out.append(case(kind, c, nd, "random", (skip + len(dens)) & 1, dens=dens, skip=skip, nb=nb))
        for skip in (0, 5):       # no density map: every scalar is dense
            for nb in ("minus1", "minus1zero", "none"):
                out.append(case(kind, c, nd, "random", skip & 1, skip=skip, nb=nb))
    # a density prefix of more than one scan tile (2050 words)
    out.append(case(CLASSIC, 24, 2050 * 64 - 7, "random", 0, dens="random", skip=5, nb="minus1", tag="longprefix"))
    return out


def all_cases():
    return shape_cases() + table_cases() + density_cases()


REPEAT_CASES = (case(CLASSIC, 16, "T+1", "random", 0, dens="random", skip=5, nb="minus1", tag="twice"),
                case(TABLE, 13, "2*spt+1", "random", 1, dens="random", skip=5, nb="minus1", tag="twice"),
                case(TABLE, 22, "2*spt+1", "random", 0, dens="random", skip=5, nb="minus1", tag="twice"))


def build(cs):
    """-> dict(kind, c, nd, raw (python ints), fmt, density (uint64 words or None), skip, n_bases, stride)"""
    rng = random.Random(case_id(cs))
    kind, c, fmt, vec = cs["kind"], cs["c"], cs["fmt"], cs["vec"]
    k = constants()
    if vec.startswith("live:"):
        vals = live_count_vector(c, int(eval(vec[5:], {}, dict(TW=k["TW"]))), rng)
    elif vec == "sparse":
        vals = sparse_tiles_vector(c, rng)
    else:
        vals = None
    nd = len(vals) if vals is not None else resolve_nd(cs)
    if vec == "over_q":
        assert fmt == 0
        raw = over_q(nd, rng)
    else:
        if vals is None:
            vals = values(vec, kind, c, nd, rng)
        if cs["stride"] == "edge":
            vals[-1] = Q - 1          # its top digit is not zero: the last record of the top row is addressed
        raw = raw_scalars(vals, fmt)
    dens = None if cs["dens"] == "none" else density_words(cs["dens"], nd, rng)
    dense_idx = np.arange(nd) if dens is None else np.flatnonzero(np.unpackbits(dens.view(np.uint8), bitorder="little")[:nd])
    skip = cs["skip"]
    if cs["nb"] == "all":
        n_bases = skip + len(dense_idx)
    elif cs["nb"] == "none":
        n_bases = skip
    else:
        assert len(dense_idx)
        n_bases = skip + len(dense_idx) - 1
        if cs["nb"] == "minus1zero":   # the dropped scalar is zero: it must flag EOF all the same
            raw[int(dense_idx[-1])] = 0
    stride = 0
    if kind == TABLE:
        Wd = model.windows(c)
        if cs["stride"] == "edge":     # (Wd - 1) stride + k comes within a few of 2^31 - 1
            stride = ((1 << 31) - 1) // Wd
            skip = stride - nd - 2
            n_bases = skip + len(dense_idx)
        elif cs["stride"] == "small":
            stride = skip + nd
        else:
            stride = skip + nd + 3
    return dict(kind=kind, c=c, nd=nd, raw=raw, fmt=fmt, density=dens, skip=skip, n_bases=n_bases, stride=stride)


def expected(inp):
    spt = spt_of(inp["c"]) if inp["kind"] == TABLE else None
    return model.stage(inp["kind"], inp["c"], inp["raw"], inp["fmt"], inp["density"], inp["skip"], inp["n_bases"], inp["stride"], spt)


# ---------------------------------------------------------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------------------------------------------------------
def scan_sizes():
    t = constants()["SCAN_TILE"]
    return (1, 2, t - 1, t, t + 1, 3 * t + 5, t * t - 1, t * t, t * t + 1)


def scan_data(pattern_name, n):
    if pattern_name == "ones":
        return np.ones(n, dtype=np.uint32)
    rng = np.random.default_rng(n)
    return rng.integers(0, max(2, ((1 << 32) - 1) // n), size=n, dtype=np.uint64).astype(np.uint32)   # total < 2^32
