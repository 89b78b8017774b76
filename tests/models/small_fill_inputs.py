"""Inputs of the small-path tests (tests/test_gpu_small_fill.py, tests/test_small_fill_model_cpu.py): shapes on the edges of the
gate, scalar vectors for the recoding, the list cap and the group law's branches, densities with cut base vectors, and
integer tables.  A case is a small dict (cheap to list at collection time); build(case) turns it into what a run needs.

A table is an integer array [Wd][row_records] (tests/models/small_fill_model.py): "mixed" draws every entry from a small pool
by (row, base) - not real multiples 2^(c w) P, so a row or column mix-up changes a bucket - and "flat" gives a whole row one
value, so equal digits meet equal points (the doubling branch) and P meets -P."""
import random

import numpy as np

from tests.models import small_fill_model as model
from tests.models import sort_stage_inputs as ssi
from tests.models import sort_stage_model as ssm

Q = ssm.Q
POOL = (1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 17)
# (c, nd): the largest fused size of the default 13-bit tables, MiMC's sizes, top_bits = 0 with 2^14 buckets, the largest fused
# sizes of narrower rows, and bucket sets below / at a workgroup's share
SHAPES_G1 = ((13, 1075), (13, 322), (13, 9), (15, 12), (10, 159), (8, 51), (5, 3), (4, 1))
SHAPES_G2 = ((13, 322), (13, 9), (15, 12), (10, 159), (8, 51), (5, 3), (4, 1))
VECTORS = ("random", "zero", "one", "qm1", "half", "halfp1", "carry0", "over_q", "equal", "capedge", "pm", "cancel")


PLAN_FIELDS = ("fused", "workgroups", "threads", "lds", "bpb", "top_bits", "sliver_load", "Wd", "entries", "nb", "MAX_SCALARS", "MAX_ENTRIES",
               "MAX_PER_BUCKET", "LIST_CAP", "LANES_PER_BUCKET", "xyzz", "affine", "guard", "sentinel", "err_bytes")


def plan_info(form, nd, c, row_records=None, flags=0):
    """bh_test_small_fill_plan as a dict of PLAN_FIELDS (rows of nd records unless told otherwise); None when the hook refuses"""
    out = np.zeros(len(PLAN_FIELDS), dtype=np.uint64)
    rc = ssi.test_lib().bh_test_small_fill_plan(form, nd, c, nd if row_records is None else row_records, flags, out.ctypes.data)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out))) if rc == 0 else None


def shapes(form):
    return SHAPES_G1 if form == 0 else SHAPES_G2


def sparse(form, c, nd):
    """G2 cases keep their non-empty buckets in the hundreds: every one is decoded with two Fp2 inversions"""
    return model.GROUP[form] == 2 and min(nd * ssm.windows(c), 1 << (c - 1)) > 1000


# ---------------------------------------------------------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------------------------------------------------------
def from_digits(c, rows):
    """{window: raw digit} -> value; windows below bit 254 only, so the value is below q"""
    assert all(w < ssi.full_windows(c) and 0 <= d < (1 << c) for w, d in rows.items())
    return sum(d << (c * w) for w, d in rows.items())


def pooled(c, nd, rng, size=150):
    """random scalars whose raw digits come from a pool of `size` magnitudes m, as m or as 2^c - m (digit -m and a carry)"""
    half = 1 << (c - 1)
    pool = [rng.randrange(1, half) for _ in range(size)] + [half]
    out = []
    for _ in range(nd):
        rows = {}
        for w in range(ssi.full_windows(c) - 1):
            m = rng.choice(pool)
            r = rng.randrange(4)
            rows[w] = 0 if r == 0 else m if r < 3 or m == half else (1 << c) - m
        out.append(from_digits(c, rows))
    return out


def cap_edges(c, nd, cap):
    """one bucket with exactly cap entries, one with cap + 1, one with cap - 1 (as far as nd full windows have room)"""
    slots = [(i, w) for w in range(ssi.full_windows(c)) for i in range(nd)]
    half = 1 << (c - 1)
    want = [(1, cap), (min(2, half), cap + 1), (min(3, half), cap - 1)]
    rows = [dict() for _ in range(nd)]
    pos = 0
    for d, count in want:
        for i, w in slots[pos:pos + count]:
            rows[i][w] = d
        pos += count
    return [from_digits(c, r) for r in rows]


def values(vec, form, c, nd, rng):
    """nd reduced scalar values"""
    half = 1 << (c - 1)
    if vec == "random":
        return pooled(c, nd, rng) if sparse(form, c, nd) else [rng.randrange(Q) for _ in range(nd)]
    if vec in ("zero", "one", "qm1", "half", "halfp1", "carry0"):
        return ssi.values(vec, ssi.TABLE, c, nd, rng)
    if vec == "equal":      # every bucket that is hit holds nd entries: past the list's cap from nd = 25 on
        return [from_digits(c, {w: rng.randrange(1, 1 << c) for w in range(0, ssi.full_windows(c), 3)})] * nd
    if vec == "capedge":
        return cap_edges(c, nd, model.LIST_CAP)
    d = min(3, half - 1) if half > 1 else 1
    if vec == "pm":         # digits d and -d in row 0 (the carry of 2^c - d lands in row 1): a bucket holds P and -Q
        return [d if i % 3 else (1 << c) - d for i in range(nd)]
    if vec == "cancel":     # with a flat table: + + + + - - - - over the scalars - every sub-worker of the scan meets P, then -P
        return [d if i % 8 < 4 else (1 << c) - d for i in range(nd)]
    raise ValueError(vec)


def over_q(form, c, nd, rng):
    raw = ssi.over_q(nd, rng)
    return raw[:32] + [0] * (nd - 32) if sparse(form, c, nd) and nd > 32 else raw


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
def table(kind, Wd, row_records):
    w = np.arange(Wd, dtype=np.int64)[:, None]
    k = np.arange(row_records, dtype=np.int64)[None, :]
    if kind == "flat":
        return np.broadcast_to(np.array(POOL, dtype=np.int64)[w % 3], (Wd, row_records)).copy()
    return np.array(POOL, dtype=np.int64)[(5 * w + 3 * k + (w * k) % 7) % len(POOL)]


def consistent_table(c, bases):
    """t[w][k] = 2^(c w) bases[k]: over it sum_d d bucket_d is the multiexp itself"""
    return [[b << (c * w) for b in bases] for w in range(ssm.windows(c))]


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def case(form, c, nd, vec, fmt, dens="none", skip=0, nb="all", tab="mixed", ident="none"):
    return dict(form=form, c=c, nd=nd, vec=vec, fmt=fmt, dens=dens, skip=skip, nb=nb, tab=tab, ident=ident)


def case_id(cs):
    parts = [model.FORMS[cs["form"]], "c%d" % cs["c"], "n%d" % cs["nd"], cs["vec"], "mont" if cs["fmt"] else "canon"]
    if cs["dens"] != "none" or cs["skip"] or cs["nb"] != "all":
        parts += [cs["dens"], "skip%d" % cs["skip"], "nb-" + cs["nb"]]
    if cs["tab"] != "mixed":
        parts.append(cs["tab"])
    if cs["ident"] != "none":
        parts.append("ident-" + cs["ident"])
    return "-".join(parts)


def vector_cases(form):
    """every shape x every vector, the formats taking turns; random and halfp1 in both"""
    out = []
    for c, nd in shapes(form):
        for j, vec in enumerate(VECTORS):
            fmt = 0 if vec == "over_q" else (j + c) & 1
            tab = "flat" if vec == "cancel" else "mixed"
            out.append(case(form, c, nd, vec, fmt, tab=tab))
            if vec in ("random", "halfp1"):
                out.append(case(form, c, nd, vec, 1 - fmt))
        out.append(case(form, c, nd, "equal", c & 1, tab="flat"))   # equal points under equal digits: the doubling branch
    return out


def density_cases(form):
    out = []
    for c, nd in ((13, 322), (10, 159)):
        full = c == 13
        for dens in ssi.DENSITIES:
            if not full and dens not in ("random", "bit64", "bitlast"):
                continue
            for skip in (0, 5):
                out.append(case(form, c, nd, "random", (skip + len(dens)) & 1, dens=dens, skip=skip))
            if dens in ("ones", "random", "bit64", "bitlast"):
                for j, nb in enumerate(("first", "mid_zero", "last")):
                    out.append(case(form, c, nd, "random", j & 1, dens=dens, skip=5 * ((j + len(dens)) & 1), nb=nb))
        for j, nb in enumerate(("first", "mid_zero", "last")):   # no density map: every scalar is dense
            out.append(case(form, c, nd, "random", j & 1, skip=5 * (j & 1), nb=nb))
    if form == 0:
        for dens, nb in (("random", "all"), ("bitlast", "all"), ("ones", "mid_zero"), ("random", "last")):
            out.append(case(form, 13, 1075, "random", 0, dens=dens, skip=5, nb=nb))
    out.append(case(form, 5, 3, "random", 1, dens="ones", skip=2, nb="last"))
    out.append(case(form, 4, 1, "one", 0, dens="bitlast", nb="first"))
    return out


def identity_cases(form):
    out = []
    for c, nd in ((13, 322), (8, 51), (5, 3)):
        out.append(case(form, c, nd, "random", c & 1, ident="hit"))
        out.append(case(form, c, nd, "random", 1 - (c & 1), ident="unseen"))
    out.append(case(form, 13, 322, "random", 0, dens="random", skip=5, nb="last", ident="hit"))
    out.append(case(form, 13, 322, "equal", 1, ident="hit"))        # an identity met on the scan of the whole table
    return out


def all_cases():
    return [cs for form in model.FORMS for cs in vector_cases(form) + density_cases(form) + identity_cases(form)]


def build(cs):
    """-> dict(form, c, nd, raw (python ints), fmt, density (uint64 words or None), skip, n_bases, row_records, table (integers))"""
    rng = random.Random(case_id(cs))
    form, c, nd, fmt, vec = cs["form"], cs["c"], cs["nd"], cs["fmt"], cs["vec"]
    Wd = ssm.windows(c)
    if vec == "over_q":
        assert fmt == 0
        raw = over_q(form, c, nd, rng)
    else:
        raw = ssi.raw_scalars(values(vec, form, c, nd, rng), fmt)
    dens = None if cs["dens"] == "none" else ssi.density_words(cs["dens"], nd, rng)
    dense_idx = np.arange(nd) if dens is None else np.flatnonzero(np.unpackbits(dens.view(np.uint8), bitorder="little")[:nd])
    skip, ndense = cs["skip"], len(dense_idx)
    if cs["nb"] == "all":
        n_bases = skip + ndense
    elif cs["nb"] == "first":          # before the first dense entry: every dense scalar is past the end
        n_bases = skip
    elif cs["nb"] == "last":           # only the last dense entry is
        n_bases = skip + max(ndense - 1, 0)
    else:                              # in the middle, and the first entry past the end is a zero scalar: EOF all the same
        assert cs["nb"] == "mid_zero"
        n_bases = skip + ndense // 2
        if ndense:
            raw[int(dense_idx[ndense // 2])] = 0
    row_records = skip + nd + 3
    tab = table(cs["tab"], Wd, row_records)
    out = dict(form=form, c=c, nd=nd, raw=raw, fmt=fmt, density=dens, skip=skip, n_bases=n_bases, row_records=row_records, table=tab)
    if cs["ident"] != "none":
        m = expected(out)
        used = np.zeros((Wd, row_records), dtype=bool)   # records under a non-zero digit of a live scalar
        for i in np.flatnonzero(m["live"]):
            used[np.flatnonzero(m["dig"][:, i]), int(m["kidx"][i])] = True
        if cs["ident"] == "hit":
            ws, ks = np.nonzero(used)
            assert len(ws)
            for j in sorted({0, len(ws) // 2, len(ws) - 1}):
                tab[ws[j], ks[j]] = 0
        else:                                            # under zero digits, in rows of scalars that are not live, behind n_bases
            tab[~used] = 0
    return out


def expected(inp):
    return model.fill(inp["c"], inp["raw"], inp["fmt"], inp["density"], inp["skip"], inp["n_bases"], inp["table"])


# ---------------------------------------------------------------------------------------------------------------------------
# the error-resolution pass
# ---------------------------------------------------------------------------------------------------------------------------
RESOLVE_STRIDES = ((1, 96), (1, 128), (2, 192))


def resolve_cases():
    """(group, stride, fmt, nd, density, ref_n, where the identities sit)"""
    out = []
    for group, stride in RESOLVE_STRIDES:
        for fmt in (0, 1):
            for nd, dens, ref_n in ((300, "none", 0), (300, "random", 0), (300, "random", 1 << 20), (70, "bit64", 0), (20, "ones", 0), (300, "ones", 2981)):
                for where in ("none", "before", "at", "after", "low_only", "not_dense"):
                    if where == "not_dense" and dens in ("none", "ones"):
                        continue
                    out.append(dict(group=group, stride=stride, fmt=fmt, nd=nd, dens=dens, ref_n=ref_n, where=where))
    return out


def resolve_id(cs):
    return "g%d-s%d-%s-n%d-%s-ref%d-%s" % (cs["group"], cs["stride"], "mont" if cs["fmt"] else "canon", cs["nd"], cs["dens"], cs["ref_n"], cs["where"])


def build_resolve(cs):
    """scalars that straddle the top window - 2^lo_ref - 1, 2^lo_ref, q - 1, 0, and (canonical) q + 2^lo_ref - 1, which is over q
    and reduces to a value below the window - with the base vector cut in the middle and identity bases placed by `where`:
    before / at / after the first entry past the end (under a scalar with top bits), under scalars without top bits only, or
    under bits the density leaves out"""
    rng = random.Random(resolve_id(cs))
    nd, fmt = cs["nd"], cs["fmt"]
    lo = model.lo_ref(cs["ref_n"] or nd)
    special = [(1 << lo) - 1, 1 << lo, Q - 1, 0, (1 << lo) + 5, rng.randrange(1 << lo)]
    vals = [special[rng.randrange(len(special))] for _ in range(nd)]
    if fmt == 0:
        for i in range(3, nd, 11):          # over q (below): the pass looks at the reduced value
            vals[i] = (1 << lo) - 1

    def raw_of(vals):
        raw = ssi.raw_scalars(vals, fmt)
        if fmt == 0:
            for i in range(3, nd, 11):
                if vals[i] == (1 << lo) - 1:
                    raw[i] = Q + vals[i]
        return raw

    raw = raw_of(vals)
    dens = None if cs["dens"] == "none" else ssi.density_words(cs["dens"], nd, rng)
    bits = np.ones(nd, dtype=np.uint8) if dens is None else np.unpackbits(dens.view(np.uint8), bitorder="little")[:nd]
    dense_idx = np.flatnonzero(bits)
    skip = 3
    n_bases = skip + max(1, (len(dense_idx) + 1) // 2)      # the dense entries from (len + 1) // 2 on are past the end
    prefix = None
    if dens is not None:
        pop = np.unpackbits(dens.view(np.uint8)).reshape(-1, 64).sum(axis=1)
        prefix = np.concatenate([[0], np.cumsum(pop)]).astype(np.uint32)
    rank = {int(i): skip + r for r, i in enumerate(dense_idx)}       # base index of dense scalar i
    top = [i for i in dense_idx if vals[i] >> lo]
    low = [i for i in dense_idx if not vals[i] >> lo]
    ident = np.zeros(skip + len(dense_idx) + 2, dtype=bool)   # a record for every dense scalar, those past the end included
    where = cs["where"]
    if where == "before":
        inside = [i for i in dense_idx if rank[i] < n_bases]
        j = inside[len(inside) // 2]
        vals[j] = 1 << lo
        ident[rank[j]] = True
        raw = raw_of(vals)
    elif where == "at":
        # the last base inside the vector, under a scalar WITHOUT top bits, and the record right behind the vector, where the
        # first entry past the end - a scalar with top bits - would look
        ident[n_bases - 1] = ident[n_bases] = True
        for i in dense_idx:
            if rank[i] == n_bases - 1:
                vals[i] = (1 << lo) - 1
            if rank[i] == n_bases:
                vals[i] = 1 << lo
        raw = raw_of(vals)
    elif where == "after":
        ident[n_bases:] = True               # every record behind the vector, every scalar that would look there with top bits
        for i in dense_idx:
            if rank[i] >= n_bases:
                vals[i] = Q - 1
        raw = raw_of(vals)
    elif where == "low_only":
        for i in low:
            if rank[i] < n_bases:
                ident[rank[i]] = True
    elif where == "not_dense":
        ident[:skip] = True                  # the skipped bases, which no scalar of this job owns
        # ... and the base a scalar WITH top bits would own if the density counted it: its owner has none
        before = np.cumsum(bits) - bits
        for i in np.flatnonzero(bits == 0):
            k = skip + int(before[i])
            owner = [j for j in dense_idx if rank[j] == k]
            if k < n_bases and owner:
                vals[i], vals[owner[0]] = 1 << lo, (1 << lo) - 1
                ident[k] = True
                break
        raw = raw_of(vals)
    return dict(group=cs["group"], stride=cs["stride"], fmt=fmt, nd=nd, raw=raw, density=dens, prefix=prefix, skip=skip, n_bases=n_bases,
                ident=ident, ref_n=cs["ref_n"], lo=lo)
