"""The one-launch small path and the error-resolution pass on their own (run with `pytest -m gpu` on a MI355X):
msm_small_fill_kernel in its four instantiations, launched once by the function msm_enqueue launches it with as the shipped
plans say (bh_test_small_fill_dev), over the inputs of tests/models/small_fill_inputs.py - shapes on the edges of the gate,
scalars for the recoding, the list cap and its table-scan fallback, P and -P and equal points in one bucket, densities with
cut base vectors, identity records under non-zero and under zero digits - and msm_err_resolve_kernel in both groups and at
every stride (bh_test_err_resolve_dev).

Everything the kernels write is compared with tests/models/small_fill_model.py: every one of the 2^(c-1) raw bucket records
(coordinates below 2p, ZZ^3 = ZZZ^2 - gm.decode asserts it - and the model's point, the identity for an empty or cancelled
bucket), every word of ErrFlags, the word prefix (untouched without a density), and the guard bytes behind every buffer.
Integer work: exact equality, no tolerance."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import group_model as gm  # noqa: E402
from tests.models import bucket_stage_model as bsm  # noqa: E402
from tests.models import small_fill_inputs as inputs  # noqa: E402
from tests.models import small_fill_model as model  # noqa: E402
from tests.models import sort_stage_inputs as ssi  # noqa: E402
from tests.models import sort_stage_model as ssm  # noqa: E402

GUARDS = ("pts", "word_prefix", "err", "scalars", "density", "table")
RESOLVE_GUARDS = ("scalars", "density", "word_prefix", "bases", "err")
ERR_WORDS = ("eof", "ident", "ident_top", "nlong", "nbig", "npieces", "madds", "zeros")


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    return ssi.test_lib()


def ptr(a):
    return None if a is None else a.ctypes.data


_records = {}


def pool_records(g, arec):
    """the affine record of v * generator for every integer a table holds; row 0 of the array is the identity"""
    if g not in _records:
        top = max(inputs.POOL)
        recs = [gm.affine_record(g, bsm.point(g, v)) for v in range(top + 1)]
        _records[g] = gm._pack(recs)
        assert _records[g].shape == (top + 1, arec) and not _records[g][0].any()
    return _records[g]


def run(lib, worker, inp):
    """-> (plan, pts rows, word_prefix or None, ErrFlags as a dict); asserts the guards"""
    form, c, nd = inp["form"], inp["c"], inp["nd"]
    p = inputs.plan_info(form, nd, c, inp["row_records"])
    assert p is not None and p["fused"] == 1, "the shipped plan does not fuse this shape"
    g = model.GROUP[form]
    table = np.ascontiguousarray(pool_records(g, p["affine"])[inp["table"].reshape(-1)])
    scalars = ssm.to_words(inp["raw"])
    pts = np.full(p["nb"] * p["xyzz"], 0x5C, dtype=np.uint8)
    err = np.full(p["err_bytes"], 0x5C, dtype=np.uint8)
    nwords = (nd + 63) // 64
    prefix = None if inp["density"] is None else np.zeros(nwords + 1, dtype=np.uint32)
    guards = np.zeros(len(GUARDS), dtype=np.uint32)
    rc = lib.bh_test_small_fill_dev(worker.ctx, form, c, ptr(scalars), inp["fmt"], nd, ptr(inp["density"]), inp["skip"], inp["n_bases"],
                                    ptr(table), inp["row_records"], ptr(pts), ptr(prefix), ptr(err), ptr(guards))
    assert rc == 0
    for name, ok in zip(GUARDS, guards):
        assert ok == 1, "bytes behind %s were written" % name
    return p, pts.reshape(p["nb"], p["xyzz"]), prefix, dict(zip(ERR_WORDS, struct.unpack("<6I2Q", err.tobytes())))


def check(inp, p, rows, prefix, err, tag):
    m = inputs.expected(inp)
    g = model.GROUP[inp["form"]]
    want_err = dict.fromkeys(ERR_WORDS, 0)
    want_err.update(eof=m["eof"], ident=m["ident"])
    assert err == want_err, (tag, "ErrFlags", err)
    if inp["density"] is not None:
        assert (prefix == m["prefix"]).all(), (tag, "word_prefix", prefix, m["prefix"])
    written = np.flatnonzero(rows.any(axis=1))
    # an all-zero record is the identity; every other one is decoded
    for b in written:
        rec = gm._unpack(rows[b], 1)[0]
        assert all(v < 2 * gm.P for v in rec), (tag, "bucket", b + 1, "a coordinate is not below 2p")
        bucket = m["buckets"].get(int(b) + 1)
        assert gm.decode(g, rec) == bsm.point(g, bucket["sum"] if bucket else 0), (tag, "bucket", int(b) + 1, bucket and bucket["entries"][:8])
    for d, bucket in m["buckets"].items():
        assert bucket["sum"] == 0 or rows[d - 1].any(), (tag, "bucket", d, "is empty")
    print(tag, "buckets %d non-empty %d overflowing %d eof %d ident %d" % (
        p["nb"], len(written), sum(b["overflow"] for b in m["buckets"].values()), m["eof"], m["ident"]))
    return m


@pytest.mark.parametrize("case", inputs.all_cases(), ids=inputs.case_id)
def test_small_fill_against_the_integer_model(worker, lib, case):
    inp = inputs.build(case)
    p, rows, prefix, err = run(lib, worker, inp)
    m = check(inp, p, rows, prefix, err, inputs.case_id(case))
    c, nd = case["c"], case["nd"]
    # the case reaches what it was built for
    if case["nb"] in ("first", "mid_zero", "last") and not (case["dens"] == "zeros"):
        assert m["eof"] == 1
    if case["ident"] != "none":
        assert m["ident"] == (1 if case["ident"] == "hit" else 0)
    if case["vec"] in ("equal", "one", "half") and nd > model.LIST_CAP and case["dens"] == "none" and case["nb"] == "all":
        assert m["buckets"] and all(b["overflow"] for b in m["buckets"].values())
    if case["vec"] == "capedge" and nd * ssi.full_windows(c) >= 3 * model.LIST_CAP:
        assert sorted(len(b["entries"]) for b in m["buckets"].values()) == [model.LIST_CAP - 1, model.LIST_CAP, model.LIST_CAP + 1]
    if case["vec"] == "cancel" and nd >= 8:   # a sub-worker's running sum returns to the identity half-way
        flat = m["dig"].reshape(-1)
        runs = [np.cumsum(np.sign(flat[part])) for b in m["buckets"].values() for part in b["subs"] if len(part) > 1]
        assert any((r[1:] == 0).any() for r in runs)
    if case["vec"] == "halfp1":
        assert (m["dig"] < 0).any()
    if (c, nd) in ((13, 1075), (15, 12), (10, 159), (8, 51), (5, 3), (4, 1)):
        assert inputs.plan_info(case["form"], nd + 1, c)["fused"] == 0, "the shape sits on the gate's edge"
    if (c, nd) == (15, 12):
        assert p["top_bits"] == 0 and p["nb"] == 16384
    if (c, nd) == (5, 3):
        assert p["nb"] <= p["bpb"] and (p["nb"] == p["bpb"]) == (case["form"] == 1)


def test_two_runs_decode_alike(worker, lib):
    """the order inside a list follows the atomics: the records may differ between runs, the points may not"""
    inp = inputs.build(inputs.case(0, 13, 322, "random", 1, dens="random", skip=5, nb="last"))
    p, first, prefix, err = run(lib, worker, inp)
    check(inp, p, first, prefix, err, "first")
    _, second, prefix2, err2 = run(lib, worker, inp)
    check(inp, p, second, prefix2, err2, "second")
    assert err == err2 and (prefix == prefix2).all()


def test_hook_refuses_what_could_leave_the_buffers(worker, lib):
    """validated on the host, before any launch: nothing is written to the output buffers"""
    nd, c = 70, 13
    raw = ssm.to_words([5] * nd)
    big = np.full(1 << 20, 0x5C, dtype=np.uint8)
    table = np.zeros(20 * (nd + 3) * 192, dtype=np.uint8)
    dens = ssi.density_words("ones", nd, None)

    def rc(form=0, c_=c, nd_=nd, fmt=0, scalars=raw, density=None, prefix=False, skip=0, n_bases=nd, rows=nd + 3):
        r = lib.bh_test_small_fill_dev(worker.ctx, form, c_, ptr(scalars), fmt, nd_, density, skip, n_bases, ptr(table), rows, ptr(big),
                                       ptr(big) if prefix else None, ptr(big), ptr(big))
        assert r == 0 or (big == 0x5C).all()
        return r

    assert rc() == 0
    big[:] = 0x5C
    assert rc(form=4) != 0 and rc(form=-1) != 0
    assert rc(fmt=2) != 0
    assert rc(nd_=0) != 0
    assert rc(c_=16) != 0 and rc(c_=3) != 0                    # widths nothing fuses for
    assert rc(c_=12, nd_=96, scalars=ssm.to_words([5] * 96), n_bases=96, rows=99) != 0   # one past the largest fused size
    assert rc(n_bases=nd + 4) != 0                             # a base cursor could leave its row
    assert rc(skip=1 << 31) != 0
    assert rc(rows=(1 << 16) + 1) != 0
    assert rc(fmt=1, scalars=ssm.to_words([ssm.Q] + [5] * (nd - 1))) != 0   # a Montgomery scalar that is no field element
    assert rc(prefix=True) != 0                                # a prefix buffer without a density map
    assert rc(density=ptr(dens)) != 0                          # ... and the other way round


# ---------------------------------------------------------------------------------------------------------------------------
# the error-resolution pass
# ---------------------------------------------------------------------------------------------------------------------------
def run_resolve(lib, worker, inp, preset):
    g, stride = inp["group"], inp["stride"]
    arec = 96 if g == 1 else 192
    point = gm._pack([gm.affine_record(g, bsm.point(g, 7))])[0]
    bases = np.zeros((len(inp["ident"]), stride), dtype=np.uint8)
    bases[~inp["ident"], :arec] = point
    bases[:, arec:] = 0xEE                                     # the padding of a 128-byte record is not part of the point
    scalars = ssm.to_words(inp["raw"])
    err = np.frombuffer(struct.pack("<6I2Q", *preset), dtype=np.uint8).copy()
    guards = np.zeros(len(RESOLVE_GUARDS), dtype=np.uint32)
    rc = lib.bh_test_err_resolve_dev(worker.ctx, g, ptr(scalars), inp["fmt"], inp["nd"], ptr(inp["density"]), ptr(inp["prefix"]), inp["skip"],
                                     inp["n_bases"], ptr(bases), len(inp["ident"]), stride, inp["ref_n"], ptr(err), ptr(guards))
    assert rc == 0
    for name, ok in zip(RESOLVE_GUARDS, guards):
        assert ok == 1, "bytes behind %s were written" % name
    return struct.unpack("<6I2Q", err.tobytes())


@pytest.mark.parametrize("case", inputs.resolve_cases(), ids=inputs.resolve_id)
def test_error_pass_against_the_model(worker, lib, case):
    inp = inputs.build_resolve(case)
    want = model.err_resolve(inp["raw"], inp["fmt"], inp["density"], inp["prefix"], inp["skip"], inp["n_bases"], inp["ident"],
                             inp["ref_n"] or inp["nd"])
    assert lib.bh_test_err_resolve_lo_ref(inp["ref_n"] or inp["nd"]) == inp["lo"]
    assert want == (1 if case["where"] == "before" else 0)
    print(inputs.resolve_id(case), "lo_ref %d identities %d ident_top %d" % (inp["lo"], int(inp["ident"].sum()), want))
    # from zeroed flags, and from flags whose every other word is set: only ident_top may change
    assert run_resolve(lib, worker, inp, (0,) * 8) == (0, 0, want, 0, 0, 0, 0, 0)
    preset = (1, 1, 0, 0x11111111, 0x22222222, 0x33333333, 0x4444444455555555, 0x6666666677777777)
    assert run_resolve(lib, worker, inp, preset) == preset[:2] + (want,) + preset[3:]
    if want == 0:
        stays = preset[:2] + (1,) + preset[3:]
        assert run_resolve(lib, worker, inp, stays) == stays   # the pass only ever sets the word


def test_error_pass_hook_refusals(worker, lib):
    buf = np.full(1 << 16, 0x5C, dtype=np.uint8)
    raw = ssm.to_words([5] * 9)
    err = np.zeros(40, dtype=np.uint8)
    g = np.zeros(5, dtype=np.uint32)

    def rc(group=1, stride=96, fmt=0, nd=9, scalars=raw, n_bases=9, density=None, prefix=None, skip=0, records=12):
        return lib.bh_test_err_resolve_dev(worker.ctx, group, ptr(scalars), fmt, nd, density, prefix, skip, n_bases, ptr(buf), records, stride, 0,
                                           ptr(err), ptr(g))

    assert rc() == 0
    assert rc(stride=192) != 0 and rc(stride=100) != 0 and rc(group=2, stride=96) != 0 and rc(group=2, stride=128) != 0 and rc(group=3) != 0
    assert rc(group=2, stride=192) == 0 and rc(stride=128) == 0
    assert rc(fmt=2) != 0 and rc(nd=0) != 0 and rc(n_bases=0) != 0 and rc(n_bases=13) != 0 and rc(records=(1 << 20) + 1) != 0 and rc(skip=1 << 31) != 0
    assert rc(fmt=1, scalars=ssm.to_words([ssm.Q] * 9)) != 0
    dens = ssi.density_words("ones", 9, None)
    assert rc(density=ptr(dens)) != 0 and rc(prefix=ptr(buf)) != 0
    assert not err.any()
