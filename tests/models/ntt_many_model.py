"""Executable model of the batched transform of bellman_amd/csrc/fft.hip (ntt_pass_kernel<ONE, true>, ntt_run_many) and of
its launch plan (csrc/fft_plan.hpp fft_many_plan / fft_many_block): k vectors a stride apart,

  * single-pass sizes PACKED: a tile holds V = 2^(log_tile - log_n) vectors, one per column - rows contiguous, the column
    stride is the vector stride, coset / 1/n factors indexed by the row only, dead columns of the last tile untouched;
  * multi-pass sizes: one launch per pass over (tile, vector), the workgroups of one tile neighbours (on one XCD where the
    tile order is XCD-aware), ping-pong through a scratch of S vectors, ceil(k / S) sub-batches one after the other.

The in-tile register steps, the pass split and the step groups are those of tests/models/ntt_model.py (imported, not
restated).  `log_tile` / `max_r` shrink the tile so that every plan is reachable over a toy field at Python speed.  A launch
is the 20-word record bh_test_fft_many_plan returns (FIELDS), so the library's own plans replay through `check_plan_coverage`
as well."""

import numpy as np

from tests.models.ntt_model import brev, ntt_step, plan_passes, step_groups

FIELDS = ("grid", "threads", "one_level", "first_vec", "n_vec", "in_scratch", "out_scratch", "in_stride", "out_stride",
          "log_n", "s", "r", "log_c", "is_last", "r0", "L", "r1", "xcd_swizzle", "log_v", "pass")


def pass_geo(log_n, r, p, s, log_tile):
    """the geometry of pass p (fft_plan.hpp pass_geo)"""
    L, last = len(r), p == len(r) - 1
    log_c = log_tile - r[p]
    if L == 1:
        log_c = 0
    elif last:
        log_c = min(log_c, r[0])
    else:
        log_c = min(log_c, log_n - s - r[p])
    tiles = (1 << log_n) >> (r[p] + log_c)
    return dict(log_n=log_n, s=s, r=r[p], log_c=log_c, is_last=int(last), r0=r[0], L=L, r1=r[1] if L > 1 else 0,
                xcd_swizzle=int(tiles >= 64 and tiles % 8 == 0))


def many_plan(log_n, k, stride, scratch_vectors, one_level, log_tile=11, max_r=11, max_grid=1 << 30, threads=(256, 512)):
    """the launches of one batched transform: a restatement of fft_many_plan"""
    r = plan_passes(log_n, max_r)
    L, n = len(r), 1 << log_n
    out = []
    if L == 1:
        log_v = log_tile - log_n
        per_launch = min(max_grid << log_v, 1 << 31)
        for v0 in range(0, k, per_launch):
            nv = min(per_launch, k - v0)
            geo = pass_geo(log_n, r, 0, 0, log_tile)
            geo["log_c"] = log_v
            out.append(dict(geo, grid=-(-nv >> log_v), threads=threads[0], one_level=0, first_vec=v0, n_vec=nv, in_scratch=0,
                            out_scratch=0, in_stride=stride, out_stride=stride, log_v=log_v, **{"pass": 0}))
        return out
    tiles = n >> log_tile
    group = min(max(scratch_vectors, 1), max_grid // tiles)
    for v0 in range(0, k, group):
        nv = min(group, k - v0)
        s = 0
        for p in range(L):
            out.append(dict(pass_geo(log_n, r, p, s, log_tile), grid=tiles * nv, threads=threads[1] if one_level else threads[0],
                            one_level=int(bool(one_level)), first_vec=v0, n_vec=nv, in_scratch=int(p != 0), out_scratch=int(p != L - 1),
                            in_stride=n if p != 0 else stride, out_stride=n if p != L - 1 else stride, log_v=0, **{"pass": p}))
            s += r[p]
    return out


def many_block(b, grid, n_vec, xcd_swizzle):
    """block -> (tile, vector of the launch) of a multi-pass launch (fft_many_block); b may be a numpy array"""
    if xcd_swizzle:
        per_xcd, slot = (grid // n_vec) >> 3, b >> 3
        return (b & 7) * per_xcd + slot // n_vec, slot % n_vec
    return b // n_vec, b % n_vec


def tile_geo(g, t):
    """where tile t of a pass is (fft.hip tile_geo): (base, in_row_stride, in_col_stride, out_base, out_row_stride,
    out_col_stride, jp0); t may be a numpy array"""
    n = 1 << g["log_n"]
    if not g["is_last"]:
        logM = g["log_n"] - g["s"] - g["r"]
        tpb = (1 << logM) >> g["log_c"]
        jp0 = (t % tpb) << g["log_c"]
        base = ((t // tpb) << (g["log_n"] - g["s"])) + jp0
        return base, 1 << logM, 1, base, 1 << logM, 1, jp0
    if g["L"] == 1:
        return 0 * t, 1, 0, 0 * t, 1, 0, 0 * t
    groups = (1 << g["r0"]) >> g["log_c"]
    mid, k00 = t // groups, (t % groups) << g["log_c"]
    M0 = n >> g["r0"]
    return k00 * M0 + (mid << g["r"]), 1, M0, k00 + (mid << g["r0"]), 1 << (g["log_n"] - g["r"]), 1, 0 * t


def _covers(addr, n_vec, stride, n, what):
    """addr covers elements [0, n) of the vectors j * stride, j < n_vec, each exactly once, and nothing else"""
    assert addr.size == n_vec * n, (what, addr.size, n_vec, n)
    vec, off = addr // stride, addr % stride
    assert addr.min() >= 0 and vec.max() < n_vec and off.max() < n, what + ": outside a vector"
    seen = np.zeros(n_vec * n, dtype=bool)
    seen[vec * n + off] = True
    assert seen.all(), what + ": an element touched twice, another never"


_TILES_CHECKED = set()


def _tiles_cover_a_vector(l, log_tile):
    """the load phases and the store phases of the tiles of a multi-pass launch each touch every element of ONE vector
    exactly once (the single-vector geometry; checked once per geometry, in chunks of tiles)"""
    key = tuple(l[f] for f in ("log_n", "s", "r", "log_c", "is_last", "r0", "L", "r1")) + (log_tile,)
    if key in _TILES_CHECKED:
        return
    n, R, C = 1 << l["log_n"], 1 << l["r"], 1 << l["log_c"]
    assert R * C == 1 << log_tile, "a multi-pass tile is full"
    e = np.arange(R * C, dtype=np.int64)
    if l["is_last"]:
        row, col = e & (R - 1), e >> l["r"]
    else:
        row, col = e >> l["log_c"], e & (C - 1)
    srow, scol = e >> l["log_c"], e & (C - 1)
    seen_ld, seen_st = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    tiles = n >> log_tile
    for t0 in range(0, tiles, 1024):
        t = np.arange(t0, min(tiles, t0 + 1024), dtype=np.int64)
        base, irs, ics, ob, ors, ocs, _ = tile_geo(l, t)
        for seen, a in ((seen_ld, base[:, None] + (row * irs + col * ics)[None, :]), (seen_st, ob[:, None] + (srow * ors + scol * ocs)[None, :])):
            a = a.ravel()
            assert a.min() >= 0 and a.max() < n, "a tile reaches outside the vector"
            seen[a] = True
    # n addresses in all (tiles * 2^log_tile), every element seen: none twice
    assert tiles << log_tile == n and seen_ld.all() and seen_st.all(), "two tiles (or two lanes) share an element"
    _TILES_CHECKED.add(key)


def check_launch_coverage(l, log_tile=11):
    """the loads of a launch are elements [0, n) of its n_vec input vectors, each exactly once, and likewise its stores"""
    n, nv = 1 << l["log_n"], l["n_vec"]
    if l["L"] == 1:   # packed: block b holds vectors b * V + col, col < live; rows contiguous
        V = 1 << l["log_v"]
        assert l["grid"] == -(-nv // V) and l["log_c"] == l["log_v"] and l["r"] + l["log_v"] == log_tile and l["r"] == l["log_n"]
        ld, st = [], []
        for b in range(l["grid"]):
            cols = np.arange(min(V, nv - b * V), dtype=np.int64) + b * V
            rows = np.arange(n, dtype=np.int64)
            ld.append((cols[:, None] * l["in_stride"] + rows[None, :]).ravel())
            st.append((cols[:, None] * l["out_stride"] + rows[None, :]).ravel())
        _covers(np.concatenate(ld), nv, l["in_stride"], n, "packed loads")
        _covers(np.concatenate(st), nv, l["out_stride"], n, "packed stores")
        return
    # (tile, vector): the blocks are a bijection onto tiles x vectors, the tiles cover a vector, the vectors do not overlap
    tiles = n >> log_tile
    assert l["grid"] == tiles * nv
    b = np.arange(l["grid"], dtype=np.int64)
    t, vec = many_block(b, l["grid"], nv, l["xcd_swizzle"])
    assert t.min() >= 0 and t.max() < tiles and vec.min() >= 0 and vec.max() < nv
    seen = np.zeros(l["grid"], dtype=bool)
    seen[t * nv + vec] = True
    assert seen.all(), "two blocks work on one (tile, vector)"
    # neighbours: the blocks of one tile are consecutive in issue order - of their XCD where the order is XCD-aware
    order = (b & 7) * (l["grid"] >> 3) + (b >> 3) if l["xcd_swizzle"] else b
    tt = np.empty(l["grid"], dtype=np.int64)
    tt[order] = t
    assert (np.diff(tt.reshape(-1, nv), axis=1) == 0).all(), "the workgroups of one tile are not neighbours"
    _tiles_cover_a_vector(l, log_tile)
    assert l["in_stride"] >= n and l["out_stride"] >= n


def check_plan_coverage(plan, log_n, k, stride, scratch_vectors, log_tile=11, max_r=11, threads=(256, 512)):
    """every (vector, element) is loaded exactly once by a first pass and stored exactly once by a last pass, nothing
    outside a vector is touched, every pass between stays inside the scratch vectors of its sub-batch, and the sub-batches
    come one after the other with their passes in order"""
    n, r = 1 << log_n, plan_passes(log_n, max_r)
    L = len(r)
    next_vec, i = 0, 0
    while i < len(plan):
        first, nv = plan[i]["first_vec"], plan[i]["n_vec"]
        assert first == next_vec and nv >= 1, "sub-batches in order, without holes"
        assert L == 1 or nv <= max(scratch_vectors, 1), "a sub-batch has to fit the scratch"
        for p in range(L):
            l = plan[i + p]
            assert (l["pass"], l["first_vec"], l["n_vec"], l["L"], l["log_n"]) == (p, first, nv, L, log_n)
            assert (l["in_scratch"], l["out_scratch"]) == (int(p != 0), int(p != L - 1))
            assert l["in_stride"] == (n if l["in_scratch"] else stride) and l["out_stride"] == (n if l["out_scratch"] else stride)
            assert l["in_stride"] >= n and l["out_stride"] >= n
            assert l["r"] == r[p] and l["s"] == sum(r[:p]) and l["is_last"] == int(p == L - 1)
            assert l["threads"] == threads[l["one_level"]] and not (l["one_level"] and L == 1)
            check_launch_coverage(l, log_tile)
        next_vec, i = first + nv, i + L
    assert next_vec == k, "every vector is in a sub-batch"


def run_many(mem, scratch, plan, mod, omega, log_n, mode, log_tile, max_r, threads, gmax=3, gen=None, trace=None):
    """Runs the launches of `plan` over mem (the caller's buffer: vector j at j * stride, None in the gaps) and scratch, as
    the kernel does.  mode: 0 fft, 1 ifft, 2 coset_fft, 3 icoset_fft; omega: primitive 2^log_n-th root; gen: the coset
    generator.  trace: dict pass -> [(buffer name, address, 'ld' | 'st')]."""
    n = 1 << log_n
    inverse = mode in (1, 3)
    w = pow(omega, mod - 2, mod) if inverse else omega
    minv = pow(n, mod - 2, mod)
    ginv = pow(gen, mod - 2, mod) if gen else None
    master_bits = log_tile
    for l in plan:
        rp, log_c = l["r"], l["log_c"]
        R, C = 1 << rp, 1 << log_c
        last, first_pass = bool(l["is_last"]), l["pass"] == 0
        src, dst = (scratch if l["in_scratch"] else mem), (scratch if l["out_scratch"] else mem)
        src0 = 0 if l["in_scratch"] else l["first_vec"] * l["in_stride"]
        dst0 = 0 if l["out_scratch"] else l["first_vec"] * l["out_stride"]
        # in-tile twiddles: entry i of the master table is w_R^(i * R / 2^master_bits); only those multiples are used
        wr = pow(w, 1 << (log_n - rp), mod) if rp else 1
        scale_ = 1 << (master_bits - rp)
        master = [pow(wr, i // scale_, mod) if i % scale_ == 0 else None for i in range(1 << (master_bits - 1))]
        packed = l["L"] == 1
        seen = set()
        for b in range(l["grid"]):
            if packed:
                v0 = b << l["log_v"]
                live = min(C, l["n_vec"] - v0)
                t, vin, vout = 0, src0 + v0 * l["in_stride"], dst0 + v0 * l["out_stride"]
            else:
                t, vec = many_block(b, l["grid"], l["n_vec"], l["xcd_swizzle"])
                assert vec < l["n_vec"] and t < (n >> log_tile) and (t, vec) not in seen
                seen.add((t, vec))
                live, vin, vout = C, src0 + vec * l["in_stride"], dst0 + vec * l["out_stride"]
            base, irs, ics, ob, ors, ocs, jp0 = tile_geo(l, t)
            total = R * live
            tile = [None] * (R * C)
            for e in range(R * C):
                if e >= total:
                    continue
                if last:
                    col, row = e >> rp, e & (R - 1)
                else:
                    row, col = e >> log_c, e & (C - 1)
                gi = base + row * irs + col * ics
                at = vin + (col * l["in_stride"] if packed else 0) + gi
                v = src[at]
                if trace is not None:
                    trace.setdefault(l["pass"], []).append(("scratch" if l["in_scratch"] else "mem", at, "ld"))
                if first_pass and mode == 2:
                    v = v * pow(gen, gi, mod) % mod    # (packed: gi is the row)
                tile[(col << rp) + brev(row, rp)] = v
            sbits, first = 0, True
            for g_ in step_groups(rp, gmax):
                ntt_step(tile, total, rp, sbits, g_, first, master, master_bits, mod, threads)
                sbits += g_
                first = False
            for e in range(R * C):
                row, col = e >> log_c, e & (C - 1)
                if (col >= live) if packed else (e >= total):
                    continue
                v = tile[(col << rp) + row]
                g = ob + row * ors + col * ocs
                if not last:
                    v = v * pow(w, (((jp0 + col) * row) << l["s"]) & (n - 1), mod) % mod
                elif mode == 3:
                    v = v * pow(ginv, g, mod) % mod * minv % mod   # (packed: g is the row)
                elif mode == 1:
                    v = v * minv % mod
                at = vout + (col * l["out_stride"] if packed else 0) + g
                dst[at] = v
                if trace is not None:
                    trace.setdefault(l["pass"], []).append(("scratch" if l["out_scratch"] else "mem", at, "st"))
    return mem


def plain_dft(x, mod, omega, mode, gen):
    """mode 0..3 of a plain O(n^2) DFT over Z_mod (mod < 2^20: the sums stay below 2^63)"""
    n = len(x)
    x = np.array(x, dtype=np.int64)
    idx = np.arange(n, dtype=np.int64)
    w = pow(omega, mod - 2, mod) if mode in (1, 3) else omega
    pw = np.array([pow(w, i, mod) for i in range(n)], dtype=np.int64)
    if mode == 2:
        x = x * np.array([pow(gen, i, mod) for i in range(n)], dtype=np.int64) % mod
    out = (pw[(idx[:, None] * idx[None, :]) % n] * x[None, :] % mod).sum(axis=1) % mod if n > 1 else x.copy()
    if mode in (1, 3):
        out = out * pow(n, mod - 2, mod) % mod
    if mode == 3:
        ginv = pow(gen, mod - 2, mod)
        out = out * np.array([pow(ginv, i, mod) for i in range(n)], dtype=np.int64) % mod
    return [int(v) for v in out]
