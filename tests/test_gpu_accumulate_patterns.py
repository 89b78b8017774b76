"""The G1 bucket accumulation over small, adversarial sorted streams, through the public multiexp (`pytest -m gpu`).

msm_accumulate_kernel<FpOps, false> (csrc/msm_accumulate.cuh) adds with the mixed addition over sliced operands (ec.cuh
xyzz_madd_sliced).  An entry that opens a bucket or a chunk partial is a copy, an addition may double or cancel, and
`mixed_additions` counts exactly the additions into a non-empty accumulator: the patterns below put each of those at every
position of a chunk.

Every job here runs over an explicit window table of 10-bit rows (26 rows, 512 buckets) on 64 - 512 bases with the chunk
forced to 8 entries, so that buckets straddle chunks and the launch has 200 - 1700 lanes.  Bases are known multiples k_i G
(0: the identity record), so that a job is checked three ways:
  * the record against the restated multiexp of oracle/ (error codes included),
  * against [sum s_i k_i] G, as bench.py checks its result,
  * `mixed_additions` of bh_msm_wait_stats against the index model of tests/models: the sorted stream of
    sort_stage_model (the order inside a bucket matters once points cancel or are identities) walked by
    bucket_stage_model.window, which counts an addition exactly where the accumulator is not the identity.
Scalar patterns: all scalars equal (one run across every chunk of a row's digit); every entry in a bucket of its own (all
openers: every store of a chunk comes from a copy); buckets of exactly one and exactly two entries at every alignment to
the chunk (an opener first and last in a chunk - asserted on the model's stream); duplicated bases with equal digits (P + P:
the doubling branch), a base and its negative, and one base with opposite digits (P - P: the bucket is empty again and
its next entry is a copy); identity bases under zero and non-zero scalars; a density map with a base offset."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cref  # noqa: E402
from tests.models import bucket_stage_model as bsm  # noqa: E402
from tests.models import sort_stage_model as ssm  # noqa: E402

C, CHUNK = 10, 8
W = ssm.windows(C)
Q = cref.Q
SPT = max(1, min(512, 7168 // W))   # scalars per tile of the first sort pass (msm_stages.hip wide_scalars_per_tile)


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


_POINTS = {}


def multiple(k):
    """the affine record of k G, k any integer (0: the identity record)"""
    k %= Q
    if k not in _POINTS:
        _POINTS[k] = np.zeros(12, dtype=np.uint64) if k == 0 else cref.point_mul(1, cref.g1_generator(), k)
    return _POINTS[k]


def signed(v):
    """v mod q as the representative of least magnitude: a point and its negative then sum to the integer 0"""
    v %= Q
    return v - Q if v > Q // 2 else v


def model_additions(ks, scalars, bits, skip, chunk, lanes):
    """(mixed additions the accumulation must count, the model's window) for bases ks[i] G and canonical scalars"""
    nd, n_bases = len(scalars), len(ks)
    dens = None if bits is None else cref.density_bitmap(bits)
    st = ssm.stage(1, C, [int(s) for s in scalars], 0, dens, skip, n_bases, n_bases, spt=SPT)
    assert not st["eof"]
    stream = st["stream"]
    entries = [(int(e >> np.uint64(32)), int((e >> np.uint64(31)) & np.uint64(1)), int(e & np.uint64(0x7FFFFFFF))) for e in stream]
    # record w * n_bases + i of the table is 2^(c w) k_i G
    values = [signed(ks[i] * (1 << (C * w))) if ks[i] % Q else 0 for w in range(W) for i in range(n_bases)]
    win = bsm.window(entries, 0, values, chunk, lanes, 1 << 30, 1 << 30, 1 << 30)
    return win["madds"], win, entries


def run(worker, ks, scalars, bits=None, skip=0, expect_rc=0):
    """one job three ways (see above); returns (counters, the model's window, its entries)"""
    import bellman_amd
    from bellman_amd import UnexpectedIdentity
    from bellman_amd.multiexp import NO_SMALL_PATH

    arr = np.stack([multiple(k) for k in ks])
    sc = cref.ints_to_arr([int(s) for s in scalars], 4)
    if bits is None:
        dens, dens_c = bellman_amd.FullDensity(), None
    else:
        dens, dens_c = bellman_amd.DensityTracker(), cref.density_bitmap(bits)
        dens.bv = bits
    rc, want = cref.multiexp(1, arr, skip, dens_c, sc)
    assert rc == expect_rc
    hb = bellman_amd.Bases(worker, 1, arr)
    hb.precompute(C)
    assert hb.table_info()[:2] == (C, W)
    try:
        job = bellman_amd.multiexp(worker, hb, dens, sc, skip=skip, chunk=CHUNK, flags=NO_SMALL_PATH, stats=True)
        if expect_rc == 1:
            with pytest.raises(UnexpectedIdentity):
                job.wait()
            return None
        got, _, st = job.wait()
    finally:
        hb.release()
    assert st["window_bits"] == C and st["chunk"] == CHUNK and st["bucket_sets"] == 1
    assert np.array_equal(got, want)
    live = [int(s) for s in scalars] if bits is None else [int(s) for s, b in zip(scalars, bits) if b]
    total = sum(s * ks[skip + j] for j, s in enumerate(live)) % Q
    assert np.array_equal(got, multiple(total))
    madds, win, entries = model_additions(ks, scalars, bits, skip, CHUNK, st["chunk_lanes"])
    print("entries %d lanes %d K %d: mixed_additions %d, model %d" % (len(entries), st["chunk_lanes"], win["K"], st["mixed_additions"], madds))
    assert st["mixed_additions"] == madds
    return st, win, entries


def distinct_bases(n, seed):
    rnd = np.random.default_rng(seed)
    return [int(v) for v in rnd.integers(1, 1 << 62, n)]


def test_all_scalars_equal_one_run_across_every_chunk(worker):
    n = 64
    s = 0x5A3C9F1E7B2D4C6A8E0F1B3D5C7E9A2B4D6F8091A3B5C7D9E1F30527496B8DAC % Q
    st, win, entries = run(worker, distinct_bases(n, 1), [s] * n)
    # every bucket holds a multiple of 64 entries: with chunks of 8 each spans at least 8 chunks
    assert win["K"] == CHUNK and all(last - lane >= 7 for lane, _, last, _, _ in win["runs"]) and win["runs"]


def test_every_entry_in_a_bucket_of_its_own(worker):
    """scalars 1 .. 500: one non-zero digit each, all different - every entry is an opener, no addition at all"""
    n = 500
    st, win, entries = run(worker, distinct_bases(n, 2), list(range(1, n + 1)))
    assert st["mixed_additions"] == 0 and len(entries) == n
    assert all(end - begin == 1 for _, _, _, _, begin, end in win["partials"])


def test_buckets_of_one_and_two_entries_at_every_alignment(worker):
    """bucket b holds 1 + (b odd) entries: 3 entries per 2 buckets against chunks of 8"""
    scalars = []
    for b in range(1, 301):
        scalars += [b] * (1 + (b & 1))
    n = len(scalars)
    assert 64 <= n <= 512
    st, win, entries = run(worker, distinct_bases(n, 3), scalars)
    digits = [e[0] for e in entries]
    opener_first = opener_last = pair_split = 0
    for v in win["views"]:
        if v is None:
            continue
        begin, end, _, _, head_partial, tail_partial = v
        opener_first += not head_partial
        opener_last += end - begin > 1 and digits[end - 1] != digits[end - 2]   # the chunk's last entry opens its bucket
        pair_split += tail_partial
    assert opener_first and opener_last and pair_split
    assert st["mixed_additions"] == 150 - pair_split   # a pair cut by a chunk boundary is two copies


def test_doubling_and_cancelling(worker):
    rnd = np.random.default_rng(4)
    ks, scalars = [], []
    for j in range(40):
        k = int(rnd.integers(1, 1 << 62))
        d = 3 + 2 * j   # a small odd digit: row 0 only
        kind = j % 4
        if kind == 0:     # P, P with equal digits: the doubling branch
            ks += [k, k]
            scalars += [d, d]
        elif kind == 1:   # P, -P (the negated base) with equal digits, then a third point: identity, then a copy
            ks += [k, -k, k + 1]
            scalars += [d, d, d]
        elif kind == 2:   # one base with opposite digits: 2^c - d recodes to -d and a carry into row 1; then two more
            ks += [k, k, k + 2, k + 3]
            scalars += [d, (1 << C) - d, d, d]
        else:             # P, P, -P, -P: doubling, then two additions of which the second cancels
            ks += [k, k, -k, -k]
            scalars += [d, d, d, d]
    # and full-width scalars shared by duplicated and negated bases: the same in every row
    for j in range(12):
        k = int(rnd.integers(1, 1 << 62))
        s = int.from_bytes(rnd.bytes(32), "little") % Q
        ks += [k, k, -k, k + 5]
        scalars += [s, s, s, s]
    assert 64 <= len(ks) <= 512
    st, win, entries = run(worker, ks, scalars)
    assert any(acc == 0 and end - begin >= 2 for _, _, _, acc, begin, end in win["partials"])   # a partial that cancelled


def test_identity_bases(worker):
    n = 96
    ks = distinct_bases(n, 5)
    scalars = [int(v) for v in np.random.default_rng(6).integers(1, 1 << 40, n)]
    for i in range(0, n, 7):   # identity records under zero scalars: skipped by the digits, never loaded
        ks[i] = 0
        scalars[i] = 0
    run(worker, ks, scalars)
    # under non-zero scalars: the identity record right after an opener, between two additions, alone in its bucket
    ks2, sc2 = list(ks), list(scalars)
    for i in (1, 2, 30, 31, 32, 90):
        ks2[i] = 0
    sc2[1], sc2[2], sc2[3] = 77, 77, 77
    sc2[29], sc2[30], sc2[31], sc2[33] = 78, 78, 78, 78
    sc2[90] = 511
    run(worker, ks2, sc2, expect_rc=1)


def test_density_map_with_skip(worker):
    n = 400
    rnd = np.random.default_rng(7)
    bits = rnd.random(n) < 0.5
    bits[-1] = True
    dense = int(bits.sum())
    scalars = [int.from_bytes(rnd.bytes(32), "little") % Q if j % 3 else int(rnd.integers(0, 4)) for j in range(n)]
    run(worker, distinct_bases(3 + dense, 8), scalars, bits=bits, skip=3)
