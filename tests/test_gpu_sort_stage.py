"""Stages 1 - 3 of a multiexp on their own (run with `pytest -m gpu` on a MI355X): the density prefix, the recursive scan, the
signed-digit recoding, the 8-bit sort of the classic plan, the fused recode-and-sort of the table plan and the zero-digit
search, run once by the shipped msm_run_stages (bh_test_sort_stage_dev) over the inputs of tests/models/sort_stage_inputs.py.

Everything the kernels write is compared with tests/models/sort_stage_model.py: every word of the result array (the table
plan's from zstart on), zstart, the other pair array (what the pass before the last left there, and the sentinel behind it),
word_prefix, every word of ErrFlags, and the guard bytes behind every buffer, which the hook sizes exactly as msm_enqueue
does but without its rounding to 256 bytes.  Integer work: exact equality, no tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.models import sort_stage_inputs as inputs  # noqa: E402
from tests.models import sort_stage_model as model  # noqa: E402

GUARDS = ("pairs_a", "pairs_b", "counts", "scan_tmp", "zstart", "word_prefix", "err", "scalars")


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    return inputs.test_lib()


def ptr(a):
    return a.ctypes.data


def run(lib, worker, inp):
    """-> (plan, dict of everything the hook returns); asserts the guards"""
    kind, c, nd = inp["kind"], inp["c"], inp["nd"]
    p = inputs.plan_info(kind, nd, c, inp["stride"])
    assert p is not None and p["c"] == c and p["nd"] == nd
    npairs, nwords = p["Wd"] * nd, (nd + 63) // 64
    scalars = model.to_words(inp["raw"])
    out = dict(pairs_a=np.zeros(npairs, dtype=np.uint64), pairs_b=np.zeros(npairs, dtype=np.uint64), zstart=np.zeros(p["W"], dtype=np.uint32),
               counts=np.zeros(p["counts"] + 1, dtype=np.uint32), err=np.zeros(p["err_bytes"] // 4, dtype=np.uint32),
               word_prefix=None if inp["density"] is None else np.zeros(nwords + 1, dtype=np.uint32))
    is_b = ctypes.c_int(-1)
    guards = np.zeros(len(GUARDS), dtype=np.uint32)
    rc = lib.bh_test_sort_stage_dev(worker.ctx, kind, c, ptr(scalars), inp["fmt"], nd, None if inp["density"] is None else ptr(inp["density"]),
                                    inp["skip"], inp["n_bases"], inp["stride"], ptr(out["pairs_a"]), ptr(out["pairs_b"]), ctypes.addressof(is_b),
                                    ptr(out["zstart"]), ptr(out["counts"]), None if out["word_prefix"] is None else ptr(out["word_prefix"]),
                                    ptr(out["err"]), ptr(guards))
    assert rc == 0
    assert is_b.value in (0, 1)
    out["is_b"] = is_b.value
    for name, ok in zip(GUARDS, guards):
        assert ok == 1, "bytes behind %s were written" % name
    return p, out


def check(inp, p, out, tag):
    m = inputs.expected(inp)
    sentinel = np.uint64(int.from_bytes(bytes([p["sentinel"]]) * 8, "little"))
    passes = p["sort_passes"]
    result, other = (out["pairs_b"], out["pairs_a"]) if out["is_b"] else (out["pairs_a"], out["pairs_b"])
    # ErrFlags: zero except eof
    want_err = np.zeros_like(out["err"])
    want_err[0] = m["eof"]
    assert (out["err"] == want_err).all(), (tag, "ErrFlags", out["err"])
    assert (out["zstart"] == m["zstart"]).all(), (tag, "zstart", out["zstart"][:8], m["zstart"][:8])
    if inp["density"] is not None:
        nwords = (inp["nd"] + 63) // 64
        assert (out["word_prefix"][:nwords] == m["word_prefix"]).all(), (tag, "word_prefix")
    if inp["kind"] == inputs.CLASSIC:
        assert passes == m["passes"] and out["is_b"] == passes % 2
        got = result.reshape(p["W"], p["n"])
        bad = np.argwhere(got != m["result"])
        assert not len(bad), (tag, "sorted array: first mismatch at (window, index)", bad[0], hex(int(got[tuple(bad[0])])))
        assert (other.reshape(p["W"], p["n"]) == m["after"](passes - 1)).all(), (tag, "the array of the pass before the last")
        return m
    bits = [p["bits%d" % k] for k in range(passes)]
    assert bits == model.table_pass_bits(inp["c"]), (tag, "key bits per pass", bits)
    assert out["is_b"] == (1 if passes == 2 else 0)
    z, live, n = int(m["zstart"][0]), m["live"], p["n"]
    assert z + live == n
    got = result[z:]
    bad = np.flatnonzero(got != m["stream"])
    assert not len(bad), (tag, "sorted stream: first mismatch at", int(bad[0]), hex(int(got[bad[0]])), hex(int(m["stream"][bad[0]])))
    if passes == 1:
        assert (other == sentinel).all(), (tag, "the second pair array of a one-pass sort")
    else:
        assert (other[:live] == m["after"](sum(bits[:-1]))).all(), (tag, "the array of the pass before the last")
        assert (other[live:] == sentinel).all(), (tag, "behind the live entries of the other pair array")
    return m


@pytest.mark.parametrize("case", inputs.all_cases(), ids=inputs.case_id)
def test_sort_stage_against_the_integer_model(worker, lib, case):
    inp = inputs.build(case)
    p, out = run(lib, worker, inp)
    m = check(inp, p, out, inputs.case_id(case))
    if case["nb"] in ("minus1", "minus1zero", "none"):
        assert m["eof"] == 1
    if case["vec"].startswith("live:"):
        assert m["live"] == int(eval(case["vec"][5:], {}, dict(TW=p["WIDE_TILE"])))
    if case["vec"] == "sparse":
        assert m["live"] < p["WIDE_TILE"] and p["first_tiles"] >= 4 and (p["sort_passes"] == 1 or p["num_tiles"] >= 4)


@pytest.mark.parametrize("case", inputs.REPEAT_CASES, ids=inputs.case_id)
def test_two_runs_are_byte_identical(worker, lib, case):
    inp = inputs.build(case)
    p, first = run(lib, worker, inp)
    _, second = run(lib, worker, inp)
    check(inp, p, first, inputs.case_id(case))
    for name in ("pairs_a", "pairs_b", "zstart", "counts", "word_prefix", "err"):
        assert first[name].tobytes() == second[name].tobytes(), name
    assert first["is_b"] == second["is_b"]


def scan_ids():
    return [(pat, n) for n in inputs.scan_sizes() for pat in ("ones", "random")]


@pytest.mark.parametrize("pat,n", scan_ids(), ids=lambda v: str(v))
def test_scan_against_the_model(worker, lib, pat, n):
    k = inputs.constants()
    data = inputs.scan_data(pat, n)
    want = model.exclusive_scan(data)
    elems = ctypes.c_size_t(0)
    assert lib.bh_test_scan_dev(worker.ctx, None, n, ctypes.addressof(elems), None, None) == 0
    top, levels = model.scan_layout(n, k["SCAN_TILE"])
    assert top <= elems.value
    tmp = np.zeros(elems.value, dtype=np.uint32)
    guards = np.zeros(2, dtype=np.uint32)
    got = data.copy()
    assert lib.bh_test_scan_dev(worker.ctx, ptr(got), n, ctypes.addressof(elems), ptr(tmp), ptr(guards)) == 0
    assert guards[0] == 1, "bytes behind the data were written"
    assert guards[1] == 1, "bytes behind the scratch were written"
    bad = np.flatnonzero(got != want)
    assert not len(bad), ("first mismatch at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    sentinel_word = int.from_bytes(bytes([k["sentinel"]]) * 4, "little")
    assert (tmp == model.scan_scratch(data, k["SCAN_TILE"], elems.value, sentinel_word)).all(), ("scratch", levels)


def test_hook_refuses_what_msm_enqueue_refuses(worker, lib):
    """validated on the host, before any launch: nothing is written to the output buffers"""
    nd, c = 70, 13
    raw = model.to_words([5] * nd)
    big = np.full(1 << 16, 0x5C, dtype=np.uint8)

    def rc(kind=1, c_=c, nd_=nd, fmt=0, scalars=raw, density=None, prefix=False, skip=0, n_bases=nd, stride=nd):
        is_b = ctypes.c_int(7)
        r = lib.bh_test_sort_stage_dev(worker.ctx, kind, c_, ptr(scalars), fmt, nd_, density, skip, n_bases, stride, ptr(big), ptr(big),
                                       ctypes.addressof(is_b), ptr(big), ptr(big), ptr(big) if prefix else None, ptr(big), ptr(big))
        assert r == 0 or ((big == 0x5C).all() and is_b.value == 7)
        return r

    assert rc(c_=1) != 0 and rc(c_=25) != 0
    assert rc(nd_=0) != 0
    assert rc(fmt=2) != 0
    assert rc(kind=2) != 0
    assert rc(kind=0) != 0                                        # the classic plan has no row stride
    assert rc(stride=(1 << 31) // model.windows(c) + 1) != 0      # Wd stride >= 2^31
    assert rc(n_bases=1 << 31) != 0
    many = (1 << 21) // 128 + 1
    assert rc(c_=2, nd_=many, scalars=np.zeros((many, 8), dtype=np.uint32), n_bases=many, stride=many) != 0   # more than 2^21 entries
    assert rc(fmt=1, scalars=model.to_words([model.Q] + [5] * (nd - 1))) != 0   # a Montgomery scalar that is no field element
    assert rc(prefix=True) != 0                                   # a prefix buffer without a density map
    dens = inputs.density_words("ones", nd, None)
    assert rc(density=ptr(dens)) != 0                             # ... and the other way round
