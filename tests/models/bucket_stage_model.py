"""Stage 4 of a multiexp (bellman_amd/csrc/msm_accumulate.cuh, msm_merge.cuh: effective_chunk, chunk_view, msm_accumulate_kernel, run_last_chunk,
msm_merge_chunks_kernel and the queues the tail kernels consume) restated on plain integers, statement by statement, so that
a change there shows here.  tests/test_bucket_stage_model_cpu.py checks the model against brute force and the shipped queue
bounds against it; tests/test_gpu_bucket_stage.py compares everything the kernels write with it.

A window is a list of n entries (digit, sign, base index) - sorted by digit from position z on, anything below - and a base
is an INTEGER s standing for the point s * generator (0: the identity), so a partial sum is an integer and "the accumulator
is the identity" is "the sum is 0" (all sums stay far below the group order).  point(g, k) turns a sum into the affine
point of tests/group_model (None = identity) with gm.mul, memoised: the streams draw their bases from a small pool, so a
case's few thousand partials are a few hundred different multiples."""

from tests import group_model as gm


def effective_chunk(n, z, chunks_per_window, K):
    live = n - z
    k = (live + chunks_per_window - 1) // chunks_per_window
    floor_k = K if K < 8 else 8
    if k < floor_k:
        k = floor_k
    return k if k < K else K


def chunk_view(digits, n, z, lane, K):
    """None where the lane has no chunk, else (begin, end, d_first, d_last, head_partial, tail_partial)"""
    b = z + lane * K
    if b >= n:
        return None
    begin, end = b, min(n, b + K)
    d_first, d_last = digits[begin], digits[end - 1]
    head_partial = begin > z and digits[begin - 1] == d_first     # never look below z
    tail_partial = end < n and digits[end] == d_last
    return begin, end, d_first, d_last, head_partial, tail_partial


def run_last_chunk(digits, n, z, K, lane, d):
    nchunks = (n - z + K - 1) // K
    lo, step = lane + 1, 1
    while True:
        hi = lo + step
        if hi >= nchunks:
            hi = nchunks
            break
        if digits[z + hi * K] != d:
            break
        lo = hi
        step <<= 1
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if digits[z + mid * K] == d:
            lo = mid
        else:
            hi = mid
    return lo


def window(entries, z, scalars, K, chunks_per_window, walk, big_chunks, piece):
    """one window: entries = [(digit, sign, base index)] * n.  Returns a dict:
      K          the effective chunk length
      views      chunk_view of every lane below chunks_per_window (None: no chunk)
      partials   [(lane, digit, (kind, index), sum, begin, end)]: kind "bucket" (index = digit), "head" or "tail" (index =
                 lane): every store of the accumulate launch, in order; [begin, end) = the entries it sums
      runs       [(lane, digit, last, route, npieces)]: route "owner", "medium" or "big"
      buckets    {digit: sum} of every bucket the stage writes (its final value)
      madds, ident, zeros: what the window adds to the counters"""
    n = len(entries)
    digits = [e[0] for e in entries]
    Ke = effective_chunk(n, z, chunks_per_window, K)
    views, partials, buckets, head, tail = [], [], {}, {}, {}
    madds, ident = 0, False
    for lane in range(chunks_per_window):
        v = chunk_view(digits, n, z, lane, Ke)
        views.append(v)
        if v is None:
            continue
        begin, end, d_first, d_last, head_partial, tail_partial = v
        acc, cur, start = 0, d_first, begin
        for p in range(begin, end):
            d, sign, idx = entries[p]
            if d != cur:   # bucket `cur` ends inside this chunk
                dest = ("head", lane) if (cur == d_first and head_partial) else ("bucket", cur)
                partials.append((lane, cur, dest, acc, start, p))
                acc, cur, start = 0, d, p
            s = scalars[idx]
            if s == 0:
                ident = True
                continue
            if acc != 0:
                madds += 1
            acc += -s if sign else s
        if cur == d_first and head_partial:
            dest = ("head", lane)
        elif tail_partial:
            dest = ("tail", lane)
        else:
            dest = ("bucket", cur)
        partials.append((lane, cur, dest, acc, start, end))
    for lane, d, (kind, index), acc, _, _ in partials:
        store = buckets if kind == "bucket" else head if kind == "head" else tail
        assert index not in store, "two stores to one destination"
        store[index] = acc
    runs = []
    for lane in range(chunks_per_window):
        v = views[lane]
        if v is None:
            continue
        begin, end, d_first, d_last, head_partial, tail_partial = v
        if not tail_partial:
            continue
        if head_partial and d_first == d_last:
            continue   # a middle piece of a long bucket
        d = d_last
        last = run_last_chunk(digits, n, z, Ke, lane, d)
        if last - lane > walk:
            if last - lane > big_chunks:
                runs.append((lane, d, last, "big", (last - lane + piece) // piece))
            else:
                runs.append((lane, d, last, "medium", 0))
        else:
            runs.append((lane, d, last, "owner", 0))
        assert d not in buckets, "a run's bucket was written by the accumulation too"
        buckets[d] = tail[lane] + sum(head[j] for j in range(lane + 1, last + 1))
    return dict(K=Ke, views=views, partials=partials, runs=runs, buckets=buckets, head=head, tail=tail, madds=madds, ident=ident,
                zeros=z if views and views[0] is not None else 0)


def stage(windows, zstart, scalars, K, chunks_per_window, walk, big_chunks, piece):
    """all windows.  long_runs / big_runs: the records msm_merge_chunks_kernel queues, as sets - (w, lane, d, last) and
    (w, lane, d, last, npieces, done) with done = what BigRun::done ends at: npieces, or 0 for a one-piece run, which never
    touches the counter"""
    wins = [window(e, z, scalars, K, chunks_per_window, walk, big_chunks, piece) for e, z in zip(windows, zstart)]
    long_runs, big_runs = set(), set()
    for w, m in enumerate(wins):
        for lane, d, last, route, np_ in m["runs"]:
            if route == "medium":
                long_runs.add((w, lane, d, last))
            elif route == "big":
                big_runs.add((w, lane, d, last, np_, np_ if np_ > 1 else 0))
    return dict(windows=wins, long_runs=long_runs, big_runs=big_runs, nlong=len(long_runs), nbig=len(big_runs),
                npieces=sum(r[4] for r in big_runs), ident=1 if any(m["ident"] for m in wins) else 0,
                madds=sum(m["madds"] for m in wins), zeros=sum(m["zeros"] for m in wins))


def brute_buckets(entries, z, scalars):
    """{digit: sum of the signed bases of the live entries with that digit}"""
    out = {}
    for d, sign, idx in entries[z:]:
        out[d] = out.get(d, 0) + (-scalars[idx] if sign else scalars[idx])
    return out


_points = {}


def point(g, k):
    """k * generator of group g as an affine point of tests/group_model"""
    if k == 0:
        return None
    key = (g, abs(k))
    if key not in _points:
        a = abs(k)
        _points[key] = gm.subgroup_points(g, 4096)[a - 1] if a <= 4096 else gm.mul(g, gm.GEN[g], a)
    return _points[key] if k > 0 else gm.neg(g, _points[key])


def piece_sums(win, lane, last, npieces, piece):
    """what the pieces of a big run add up: partial 0 is the tail partial of the run's first chunk, partial t the head partial
    of chunk lane + t"""
    parts = [win["tail"][lane]] + [win["head"][j] for j in range(lane + 1, last + 1)]
    return [sum(parts[q * piece:(q + 1) * piece]) for q in range(npieces)]
