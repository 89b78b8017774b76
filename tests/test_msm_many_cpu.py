"""The plan of a many-job (bh_msm_many_plan_info: k scalar vectors over one base vector in one job) and the Python model of
its digit layout (tests/models/many_digits_model.py), without a GPU.  tests/test_gpu_msm_many.py runs the job itself."""
import ctypes
import random

import pytest

from bellman_amd import _lib
from tests.models import many_digits_model as mdm

XYZZ_BYTES = {1: 192, 2: 384}
KS = [1, 2, 3, 16, 64]
NS = [9, 64, 4113, 1 << 16]
TABLE_BITS = [0, 8, 10, 13, 16, 20]


@pytest.fixture(scope="module")
def lib():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _many_plan(lib, n, k, group, bits, num_cus=256):
    out = (ctypes.c_uint * 12)()
    rc = lib.bh_msm_many_plan_info(n, k, group, bits, num_cus, out)
    return rc, dict(zip(("c", "W", "nb", "K", "chunks", "passes", "entries", "vectors", "per_vector", "Wd", "bytes_lo", "bytes_hi"),
                        (int(x) for x in out)))


def _single_plan(lib, n, group):
    out = (ctypes.c_uint * 9)()
    assert lib.bh_msm_plan_info(n, group, 0, out) == 0
    return dict(zip(("c", "W", "nb", "K", "chunks", "passes", "lo", "hi", "Wn"), (int(x) for x in out)))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("bits", TABLE_BITS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_many_plan_shape(lib, k, n, bits, group):
    rc, p = _many_plan(lib, n, k, group, bits)
    single = _single_plan(lib, n, group)
    c = bits if bits else single["c"]
    wd = (256 + c - 1) // c
    per_vector = 1 if bits else wd
    entries = wd * n if bits else n
    W = k * per_vector
    if W * entries >= 1 << 32 or W > 65535 or W << (c - 1) >= 1 << 32:
        assert rc == -2   # BH_ERR_INVALID_ARG beyond the 32-bit limits
        return
    assert rc == 0
    assert p["c"] == c and p["Wd"] == wd and p["vectors"] == k and p["per_vector"] == per_vector
    assert p["W"] == k * p["per_vector"]
    assert p["entries"] == entries
    assert p["W"] * p["entries"] < 1 << 32
    assert p["nb"] == 1 << (c - 1)
    assert p["chunks"] == -(-entries // p["K"]) and p["K"] >= 1
    assert (p["bytes_hi"] << 32 | p["bytes_lo"]) >= p["W"] * c * XYZZ_BYTES[group]
    if not bits:
        # the classic flavour keeps the single plan's rules for the per-set entry count
        assert (p["K"], p["passes"], p["chunks"]) == (single["K"], single["passes"], single["chunks"])
    elif k == 1:
        # one vector over a table IS the table plan: one bucket set, sorted by the fused passes (up to 10 key bits each)
        tp = (ctypes.c_uint64 * 23)()
        assert lib.bh_test_sort_plan(1, n, c, n, int(group == 2), 256, tp) == 0
        assert (p["entries"], p["c"], p["W"], p["passes"]) == (tp[0], tp[1], tp[2], tp[6])
    else:
        assert p["passes"] == (c + 7) // 8   # every set by the 8-bit passes of the classic sort


def test_many_plan_refuses_what_the_pipeline_cannot_index(lib):
    assert _many_plan(lib, 1 << 16, 0, 1, 0)[0] == -2            # no vectors
    assert _many_plan(lib, 1 << 16, 1 << 16, 1, 0)[0] == -2      # more bucket sets than a grid has rows
    assert _many_plan(lib, 1 << 26, 64, 1, 0)[0] == -2           # 64 * 13 sets of 2^26 entries
    assert _many_plan(lib, 1 << 23, 64, 1, 20)[0] == -2          # 64 sets of 13 * 2^23 entries
    assert _many_plan(lib, 1 << 16, 2, 3, 0)[0] == -2            # no such group
    assert _many_plan(lib, 1 << 16, 2, 1, 25)[0] == -2           # no such table
    assert _many_plan(lib, 1 << 20, 16, 1, 20)[0] == 0


def test_many_plan_chunks_count_every_set(lib):
    """where the table rule keys on "the chip runs out of lanes" it counts the lanes of all k sets: more vectors never
    shorten the chunks, and a chip-filling count of sets reaches the average bucket"""
    for n, bits in ((1 << 12, 10), (1 << 16, 13), (1 << 14, 16)):
        ks = [_many_plan(lib, n, k, 1, bits)[1]["K"] for k in (1, 2, 4, 16, 64)]
        assert ks == sorted(ks), (n, bits, ks)
        wd = (256 + bits - 1) // bits
        assert ks[-1] <= max(8, (wd * n) >> (bits - 1)) or ks[-1] == ks[0]


# ---- the digit layout ------------------------------------------------------------------------------------------------------
def _vectors(k, nd, seed):
    rnd = random.Random(seed)
    vs = [[rnd.randrange(mdm.Q) for _ in range(nd)] for _ in range(k)]
    vs[0][1], vs[0][2], vs[0][3] = 0, 1, mdm.Q - 1
    vs[1][4] = 1 << 200
    vs[2][5] = (1 << 254) + 12345          # < q: the top window's carry
    return vs


@pytest.mark.parametrize("c", [8, 13, 16])
def test_signed_digits_recompose(c):
    rnd = random.Random(c)
    for s in [0, 1, mdm.Q - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1] + [rnd.randrange(mdm.Q) for _ in range(200)]:
        digs = mdm.signed_digits(s, c)
        assert len(digs) == (256 + c - 1) // c
        assert all(0 <= mag <= 1 << (c - 1) and (mag or not neg) for mag, neg in digs)
        assert sum((-mag if neg else mag) << (c * j) for j, (mag, neg) in enumerate(digs)) == s


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("dense", [False, True])
def test_many_digit_layout_against_brute_force(table, dense):
    """n = 70, k = 3: position and base field of pair (v, j, i), with density and skip, against a brute-force enumeration
    that never uses the closed formula."""
    nd, k, c, skip = 70, 3, 13, 7
    wd = (256 + c - 1) // c
    stride = 1000 if table else 0
    rnd = random.Random(11)
    density = [rnd.random() < 0.55 for _ in range(nd)] if dense else None
    n_dense = sum(density) if dense else nd
    n_bases = skip + n_dense - 2          # the last two dense entries run off the end of the bases
    vs = _vectors(k, nd, 5)
    pairs, eof = mdm.many_pairs(vs, c, density, skip, n_bases, stride)
    assert eof and len(pairs) == k * wd * nd
    sets = mdm.bucket_sets(pairs, k, nd, c, table)
    assert len(sets) == (k if table else k * wd) and all(len(s) == (wd * nd if table else nd) for s in sets)
    # brute force: walk the sets in their own order
    for s_idx, s in enumerate(sets):
        for pos, e in enumerate(s):
            if table:
                v, j, i = s_idx, pos // nd, pos % nd
            else:
                v, j, i = s_idx // wd, s_idx % wd, pos
            is_dense = density[i] if dense else True
            rank = sum(1 for t in range(i) if (density[t] if dense else True))
            base = skip + rank
            live = is_dense and base < n_bases
            value = vs[v][i] if live else 0
            # digit j by definition: the balanced residue of (value - lower digits) mod 2^c
            low = sum((-m if ng else m) << (c * t) for t, (m, ng) in enumerate(mdm.signed_digits(value, c)[:j]))
            r = ((value - low) >> (c * j)) % (1 << c)
            d = r - (1 << c) if r > 1 << (c - 1) else r
            assert e >> 32 == abs(d) and (e >> 31) & 1 == int(d < 0), (v, j, i)
            assert e & 0x7FFFFFFF == base + j * stride, (v, j, i)
    zs = mdm.zero_counts(sets)
    # an entry that is not live is zero in every digit column of every vector
    dead = sum(1 for i in range(nd) if not ((density[i] if dense else True) and skip + sum(1 for t in range(i) if (density[t] if dense else True)) < n_bases))
    assert dead >= 2 and all(z >= (dead * wd if table else dead) for z in zs)


def test_python_binding_exports():
    import bellman_amd

    assert bellman_amd.MANY_FORCE == 512 and callable(bellman_amd.multiexp_many)
