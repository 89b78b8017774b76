"""Stage 5 of a multiexp - the reduction of filled buckets - and its host tail, restated over plain integers
(csrc/msm_stage_plans.hpp: reduce_plan; csrc/msm_ec.cuh: launch_reduce, msm_host_tail; tests/test_reduce_stage_model_cpu.py,
tests/test_gpu_reduce_stage.py).

The launches are not rewritten here: bh_test_reduce_plan hands out the schedule of the shipped reduce_plan - every launch
launch_reduce issues, as data - and `execute` replays that schedule over integer buckets - with
tests/models/bucket_sum_model.run_job, or, where 2^22 buckets would take minutes, with an index matrix that is pinned against run_job on the small plans.  While replaying it
checks what no parity test of a whole multiexp can see: every record a job reads lies inside its buffer and was written by an
earlier launch (`pts`: is an input), every cell of rows, cols and bits is written exactly once, nothing is written outside the
planned sizes, lane counts are powers of two that fit their workgroups.  What comes out is compared with the definitions:

  rows[w][hi] = sum_lo B[w][hi 2^l + lo]      cols[w][lo] = sum_hi B[w][hi 2^l + lo]       (l = lo_bits, idx = hi 2^l + lo)
  U[w][p]     = sum of the B[w][idx] with bit p of idx set                                 T[w] = sum_idx B[w][idx]
  bits        = [W][lo_bits] U of the low bits, [W][hi_bits] U of the high bits, [W] T     (the layout msm_host_tail walks)
  tail        = sum_w 2^(c w) (sum_p 2^p U[w][p] + T[w])  =  sum_w 2^(c w) sum_idx (idx + 1) B[w][idx]"""
import ctypes

import numpy as np

from tests.models import bucket_sum_model as bsm

FORMS = {0: "g1", 1: "g2k3", 2: "g2"}
FORM_GROUP = {0: 1, 1: 2, 2: 2}
KINDS = {0: "classic", 1: "table"}
PTS, ROWCOL, PART, BITS = range(4)
BUF_NAMES = ("pts", "rowcol", "part", "bits")
PLAN_WORDS = ("c", "W", "nb", "NB", "lo_bits", "hi_bits", "two_len", "want_part", "rowcol", "part", "bits", "guard", "sentinel",
              "record", "affine", "num_cus")
JOB_WORDS = ("mode", "groups", "count", "inner", "stride", "istride", "group_shift", "splits", "lanes", "in_off", "out_off",
             "in_buf", "out_buf", "nblocks")
LAUNCH_WORDS = 4 + 3 * len(JOB_WORDS)
# workers of a wavefront by worker kind (the forms of bh_test_sum_jobs_dev): in the trees, and when every worker sums alone
TREE_PER_WAVE = {0: 64, 1: 32, 2: 64, 3: 16, 5: 8}
SOLO_PER_WAVE = {0: 64, 1: 32, 2: 64, 3: 21, 5: 8}
# (worker kind, wavefronts per workgroup) launch_sums can emit, by form
WORKERS = {0: {(0, 1), (1, 1), (1, 2), (1, 4)}, 1: {(3, 4), (5, 4)}, 2: {(2, 1)}}
SMALL = 1 << 13   # plans of at most this many buckets are replayed by bucket_sum_model.run_job as well


def query(lib, form, kind, c, num_cus, ctx=None):
    """(plan dict, [launch dict]) of bh_test_reduce_plan"""
    words = (ctypes.c_uint32 * len(PLAN_WORDS))()
    n = ctypes.c_size_t()
    raw = (ctypes.c_uint32 * (8 * LAUNCH_WORDS))()
    rc = lib.bh_test_reduce_plan(ctx, form, kind, c, num_cus, words, raw, 8, ctypes.byref(n))
    assert rc == 0, (form, kind, c, num_cus, rc)
    plan = dict(zip(PLAN_WORDS, (int(x) for x in words)), form=form, kind=kind)
    launches = []
    for k in range(n.value):
        w = [int(x) for x in raw[k * LAUNCH_WORDS:(k + 1) * LAUNCH_WORDS]]
        jobs = [dict(zip(JOB_WORDS, w[4 + q * len(JOB_WORDS):4 + (q + 1) * len(JOB_WORDS)])) for q in range(3)]
        for j in jobs:
            j["mode"] = {1: "strided", 2: "bits"}.get(j["mode"], j["mode"])
        launches.append(dict(kind=w[0], waves=w[1], blocks=w[2], max_lanes=w[3], jobs=jobs))
    return plan, launches


def sizes(plan):
    return {PTS: plan["NB"], ROWCOL: plan["rowcol"], PART: plan["part"], BITS: plan["bits"]}


def job_indices(d, g0=0, g1=None):
    """(outputs g0 .. g1, elements per output) matrix of the records a job reads, relative to in_off: partial_sum of
    bucket_sum_model over all of an output's workers, as arrays"""
    g = np.arange(g0, d["groups"] if g1 is None else g1, dtype=np.int64)
    gg = g // d["splits"]
    outer, in_idx = gg // d["inner"], gg % d["inner"]
    base = outer << d["group_shift"]
    if d["mode"] == "strided":
        ln = d["count"] // d["splits"]
        k = (g % d["splits"])[:, None] * ln + np.arange(ln, dtype=np.int64)[None, :]
        return base[:, None] + (in_idx * d["istride"])[:, None] + k * d["stride"]
    assert d["mode"] == "bits", d
    j = np.arange(d["count"] >> 1, dtype=np.int64)[None, :]
    kb = in_idx[:, None]
    return base[:, None] + (((j >> kb) << (kb + 1)) | (1 << kb) | (j & ((1 << kb) - 1)))


class PlanError(AssertionError):
    pass


def _need(cond, *what):
    if not cond:
        raise PlanError(what)


def check_job_shape(launch, j):
    """what sum_count and the kernel rely on: lanes a power of two that a workgroup holds, whole pieces, whole workgroups"""
    kind, waves = launch["kind"], launch["waves"]
    _need(launch["max_lanes"] == waves * TREE_PER_WAVE[kind], "lanes a workgroup holds", launch)
    lanes = j["lanes"]
    _need(lanes >= 1 and lanes & (lanes - 1) == 0 and lanes <= waves * TREE_PER_WAVE[kind], "lanes", launch["kind"], waves, j)
    if not j["groups"]:
        _need(j["nblocks"] == 0, "workgroups of an empty job", j)
        return
    _need(j["count"] >= 1 and j["inner"] >= 1 and j["splits"] >= 1, "empty dimension", j)
    _need(j["count"] % j["splits"] == 0 and j["groups"] % j["splits"] == 0, "uneven pieces", j)
    wpb = waves * (SOLO_PER_WAVE[kind] if lanes == 1 else TREE_PER_WAVE[kind])
    _need(j["nblocks"] == -(-j["groups"] * lanes // wpb), "workgroups", j)
    if j["mode"] == "bits":
        _need(j["splits"] == 1 and j["count"] & (j["count"] - 1) == 0 and (1 << j["inner"]) <= max(j["count"], 2), "bit sums", j)
        _need(j["count"] >= 2, "a bit sum over one element selects nothing", j)


CHUNK = 1 << 20   # records gathered at a time


def check_shapes(plan, launches):
    for li, launch in enumerate(launches):
        _need((launch["kind"], launch["waves"]) in WORKERS[plan["form"]], "worker kind", li, launch["kind"], launch["waves"])
        _need(launch["blocks"] == sum(j["nblocks"] for j in launch["jobs"]) and launch["blocks"] > 0, "workgroups of launch", li)
        for j in launch["jobs"]:
            check_job_shape(launch, j)


def access_key(launches):
    """what `execute` depends on: the descriptors without lane counts, workgroups and worker kinds"""
    skip = ("lanes", "nblocks")
    return repr([[sorted((k, v) for k, v in j.items() if k not in skip) for j in l["jobs"] if j["groups"]] for l in launches])


def execute(plan, launches, buckets, slow=None):
    """Replays the planned launches over integer buckets (an integer array of NB values).  Returns (values, written): per
    buffer an int64 array (pts: as given) and how often each cell was written.  Raises PlanError where a job leaves its
    buffers, reads a cell no earlier launch wrote, or has a malformed shape.  slow: also replay every job with
    bucket_sum_model.run_job and compare (default: plans of at most SMALL buckets)."""
    size = sizes(plan)
    _need(len(buckets) == plan["NB"], "buckets", len(buckets), plan["NB"])
    if slow is None:
        slow = plan["NB"] <= SMALL
    check_shapes(plan, launches)
    val = {b: np.zeros(n, dtype=np.int64) for b, n in size.items() if b != PTS}
    val[PTS] = np.asarray(buckets)
    written = {b: np.zeros(n, dtype=np.int8) for b, n in size.items() if b != PTS}
    for li, launch in enumerate(launches):
        results = []
        for q, j in enumerate(launch["jobs"]):   # the jobs of a launch run side by side: all read before any of them writes
            if not j["groups"]:
                continue
            ib, ob = j["in_buf"], j["out_buf"]
            _need(ib in (PTS, ROWCOL, PART) and ob in (ROWCOL, PART, BITS), "buffers", li, q, j)
            _need(j["out_off"] + j["groups"] <= size[ob], "writes outside %s" % BUF_NAMES[ob], li, q, j)
            per = j["count"] // j["splits"] if j["mode"] == "strided" else j["count"] >> 1
            step = max(1, CHUNK // max(1, per))
            out = np.empty(j["groups"], dtype=np.int64)
            for g0 in range(0, j["groups"], step):
                idx = job_indices(j, g0, min(j["groups"], g0 + step)) + j["in_off"]
                _need(idx.min() >= 0 and idx.max() < size[ib], "reads outside %s" % BUF_NAMES[ib], li, q, int(idx.max()), size[ib], j)
                if ib != PTS:   # (every bucket is an input)
                    _need((written[ib][idx] >= 1).all(), "reads a cell of %s that nothing wrote" % BUF_NAMES[ib], li, q, j)
                out[g0:g0 + len(idx)] = val[ib][idx].sum(axis=1, dtype=np.int64)
            if slow:
                data = val[ib][j["in_off"]:].tolist()
                _need(bsm.run_job(j, data, j["lanes"]) == out.tolist(), "index matrix against bucket_sum_model.run_job", li, q, j)
            results.append((ob, j["out_off"], out))
        for ob, off, out in results:
            val[ob][off:off + len(out)] = out
            written[ob][off:off + len(out)] += 1
    return val, written


def check_written_once(plan, written):
    for b, n in sizes(plan).items():   # (the plan's own sizes: `written` may come from another plan with the same accesses)
        _need(b == PTS or len(written[b]) == n, "size of %s" % BUF_NAMES[b], len(written.get(b, ())), n)
    _need((written[ROWCOL] == 1).all(), "rows / cols cells not written exactly once", np.flatnonzero(written[ROWCOL] != 1)[:8].tolist())
    _need((written[BITS] == 1).all(), "bits cells not written exactly once", np.flatnonzero(written[BITS] != 1)[:8].tolist())
    _need((written[PART] <= 1).all(), "part cells written twice", np.flatnonzero(written[PART] > 1)[:8].tolist())
    _need(bool(plan["want_part"]) == bool(plan["part"]), "a part buffer without a two-stage sum, or the reverse")


def definitions(plan, buckets):
    """rows, cols, bits from their definitions (module docstring), as flat int64 arrays in the buffers' layouts"""
    W, lo, hi = plan["W"], plan["lo_bits"], plan["hi_bits"]
    B = np.asarray(buckets).reshape(W, 1 << hi, 1 << lo)
    rows, cols = B.sum(axis=2, dtype=np.int64), B.sum(axis=1, dtype=np.int64)

    def bit_sums(v, nbits):   # (W, 2^nbits) -> (W, nbits): the sum of the entries whose index has bit p set
        idx = np.arange(v.shape[1])
        return np.stack([v[:, (idx >> p) & 1 == 1].sum(axis=1) for p in range(nbits)], axis=1) if nbits else np.zeros((W, 0), np.int64)

    # a bucket's index is hi 2^l + lo: its low bits are those of its column, its high bits those of its row
    Ulo, Uhi = bit_sums(cols, lo), bit_sums(rows, hi)
    if plan["NB"] <= 1 << 16:   # ... which the small plans check on the buckets themselves
        direct = bit_sums(B.reshape(W, -1).astype(np.int64), lo + hi)
        assert np.array_equal(direct[:, :lo], Ulo) and np.array_equal(direct[:, lo:], Uhi)
    bits = np.concatenate([Ulo.reshape(-1), Uhi.reshape(-1), rows.sum(axis=1)])
    return np.concatenate([rows.reshape(-1), cols.reshape(-1)]), bits


def tail(plan, bits):
    """msm_host_tail's walk over `bits` (any values that add and scale: Python integers here)"""
    W, c, lo, hi = plan["W"], plan["c"], plan["lo_bits"], plan["hi_bits"]
    bits = [int(v) for v in bits]
    total = 0
    for w in range(W):
        u = sum(bits[w * lo + p] << p for p in range(lo)) + sum(bits[W * lo + w * hi + p] << (lo + p) for p in range(hi))
        total += (u + bits[W * (c - 1) + w]) << (c * w)
    return total


def weighted(plan, buckets):
    """sum_w 2^(c w) sum_idx (idx + 1) B[w][idx]"""
    W, c = plan["W"], plan["c"]
    B = np.asarray(buckets).reshape(W, -1)
    weights = np.arange(B.shape[1], dtype=np.int64) + 1
    return sum(int(np.dot(B[w].astype(np.int64), weights)) << (c * w) for w in range(W))   # |B| <= 2^7: below 2^55


def check_plan(plan, launches, buckets):
    """everything above for one plan; returns (values, written, coverage facts of the plan)"""
    val, written = execute(plan, launches, buckets)
    check_written_once(plan, written)
    rowcol, bits = definitions(plan, buckets)
    _need(np.array_equal(val[ROWCOL], rowcol), "rows / cols differ from their definition", np.flatnonzero(val[ROWCOL] != rowcol)[:8].tolist())
    _need(np.array_equal(val[BITS], bits), "bits differ from their definition", np.flatnonzero(val[BITS] != bits)[:8].tolist())
    _need(tail(plan, val[BITS]) == weighted(plan, buckets), "tail model")
    return val, written, coverage(plan, launches)


def coverage(plan, launches):
    """what a plan reaches, as a set of facts (the tests assert the union over what they run)"""
    facts = {("worker", l["kind"], l["waves"]) for l in launches}
    facts.add(("want_part", bool(plan["want_part"])))
    facts.add(("t_from_cols", plan["lo_bits"] < plan["hi_bits"]))
    if plan["lo_bits"] == 0:
        facts.add(("lo_bits", 0))
    if plan["want_part"]:
        H, Lw, two = 1 << plan["hi_bits"], 1 << plan["lo_bits"], plan["two_len"]
        facts.add(("Sr>1", Lw // min(two, Lw) > 1))
        facts.add(("Sc>1", H // min(two, H) > 1))
    return facts


def seeded_buckets(plan, seed, lo=-8, hi=8):
    rng = np.random.default_rng([plan["c"], plan["kind"], plan["form"], seed])
    return rng.integers(lo, hi + 1, size=plan["NB"], dtype=np.int8)
