"""The one-launch small path of a multiexp (bellman_amd/csrc/msm_accumulate.cuh msm_small_fill_kernel, its gate small_fill_plan of
msm_stage_plans.hpp) and the error-resolution pass (msm_err_resolve_kernel, err_resolve_lo_ref) restated on plain integers,
statement by statement, so that a change there shows here.  tests/test_small_fill_model_cpu.py checks the model against brute
force and the shipped gate against it; tests/test_gpu_small_fill.py compares everything the kernels write with it.

As in bucket_stage_model.py a table record is an INTEGER s standing for the point s * generator (0: the identity), so a
bucket is an integer.  The scalar load, the density rank and the signed-digit recoding are those of sort_stage_model.py: the
kernel's own copies say the same thing (v > half: d = v - 2^c and a carry; k = skip + dense bits before i; every dense entry
checks EOF first, whatever its scalar)."""
import decimal

import numpy as np

from tests.models import sort_stage_model as ssm

# the constants of msm_stage_plans.hpp, restated: bh_test_small_fill_plan reports the shipped ones
MAX_SCALARS, MAX_ENTRIES, MAX_PER_BUCKET, LIST_CAP = 2048, 20480 + 1024, 16, 24
THREADS, LANES_PER_BUCKET = 256, 4
NO_SMALL_PATH = 8                                   # BH_MSM_NO_SMALL_PATH
FORMS = {0: "fp", 1: "fp2k3", 2: "fp2pair", 3: "fp2"}
GROUP = {0: 1, 1: 2, 2: 2, 3: 2}
# workers of a 256-thread workgroup in the shuffle trees: one lane per point, 16 lane triples or 32 lane pairs per wavefront
WORKERS = {0: 256, 1: 4 * 16, 2: 4 * 32, 3: 256}
NO_KIDX = 0xFFFFFFFF


def lds_bytes(nd, n_entries):
    """base indices, digit table (16-bit, rounded up to a word), a counter per thread, a list per thread"""
    return nd * 4 + ((n_entries * 2 + 3) & ~3) + THREADS * 4 + THREADS * LIST_CAP * 2


def gate(form, nd, c, flags=0, small_path=True, many=False):
    """small_fill_plan over the table plan of nd scalars and ceil(256 / c) rows"""
    Wd = ssm.windows(c)
    n, nb = Wd * nd, 1 << (c - 1)
    top_bits = 255 - (Wd - 1) * c
    sliver_load = 0 if top_bits >= 31 else nd >> top_bits
    lds = lds_bytes(nd, n)
    fused = (small_path and not many and nd <= MAX_SCALARS and n <= MAX_ENTRIES and n <= MAX_PER_BUCKET * nb and c <= 15 and
             lds <= 64 * 1024 and sliver_load + n // nb <= LIST_CAP // 2 and not flags & NO_SMALL_PATH)
    bpb = WORKERS[form] // LANES_PER_BUCKET
    return dict(fused=int(fused), workgroups=(nb + bpb - 1) // bpb, threads=THREADS, lds=lds, bpb=bpb, top_bits=top_bits,
                sliver_load=sliver_load, Wd=Wd, entries=n, nb=nb)


def digits(values, c):
    """signed digits [Wd][nd] (int64) of reduced scalar values: raw digit plus carry v; v > 2^(c-1) gives v - 2^c and a carry"""
    mag, sign, carry = ssm.recode(values, c)
    assert not carry.any(), "the top digit of a reduced scalar has no carry out"
    d = np.where(sign.astype(bool), -mag.astype(np.int64), mag.astype(np.int64))
    assert d.min(initial=0) >= -(1 << 15) and d.max(initial=0) < (1 << 15), "a digit is kept in a short"
    return np.ascontiguousarray(d.T)


def fill(c, raw, fmt, density_words, skip, n_bases, table, list_cap=LIST_CAP, lanes=LANES_PER_BUCKET):
    """One launch.  table[w][k]: the integer of record k of row w.  Returns a dict:
      kidx      [nd] base index of scalar i, NO_KIDX where it contributes nothing
      dig       [Wd][nd] signed digits (all zero for a scalar that is not live: it is never loaded)
      eof, ident   the two flags the kernel may set
      prefix    the ceil(nd / 64) + 1 words of word_prefix (None without a density)
      buckets   {d: dict(entries, overflow, subs, sums, sum)} for every bucket d = |digit| in [1, 2^(c-1)] with an entry:
                entries = the entry ids e = w nd + i in increasing order; overflow = the list outgrew list_cap and the workers
                scan the table; subs[s] = the entries sub-worker s adds - every 4th of the scan on the fallback route, every 4th
                list position on the list route (there the positions follow the order of the atomics: subs is one such order,
                the sum does not depend on it); sums[s] their signed sum, sum the bucket's"""
    nd = len(raw)
    Wd = ssm.windows(c)
    dense, k, live, eof, prefix = ssm.density_rank(nd, density_words, skip, n_bases)
    values = ssm.load_scalars(raw, fmt)
    values = [v if l else 0 for v, l in zip(values, live)]
    dig = digits(values, c)
    kidx = np.where(live, k, NO_KIDX).astype(np.uint64)
    if prefix is not None:   # word t: dense bits of the words before t, t = nwords included
        words = np.asarray(density_words, dtype=np.uint64)
        total = int(np.unpackbits(words.view(np.uint8)).sum())
        prefix = np.concatenate([prefix, np.array([total], dtype=np.uint32)])
    buckets, ident = {}, False
    flat = dig.reshape(-1)
    for e in np.flatnonzero(flat):
        e = int(e)
        buckets.setdefault(abs(int(flat[e])), []).append(e)
    out = {}
    for d, entries in buckets.items():
        assert 1 <= d <= (1 << (c - 1))
        overflow = len(entries) > list_cap
        subs = [entries[s::lanes] for s in range(lanes)]     # seen % lanes == sub, or list position t = sub, sub + lanes, ...
        sums = []
        for part in subs:
            acc = 0
            for e in part:
                w, i = divmod(e, nd)
                assert kidx[i] != NO_KIDX, "a scalar that is not live has all-zero digits"
                s = int(table[w][int(kidx[i])])
                if s == 0:
                    ident = True
                    continue
                acc += -s if flat[e] < 0 else s
            sums.append(acc)
        out[d] = dict(entries=entries, overflow=overflow, subs=subs, sums=sums, sum=sum(sums))
    return dict(kidx=kidx, dig=dig, live=live, eof=int(eof), ident=int(ident), prefix=prefix, buckets=out, nd=nd, Wd=Wd, c=c)


def brute_total(c, raw, fmt, density_words, skip, n_bases, bases):
    """sum over the live scalars of s_i * bases[k_i], straight from the definition (no digits)"""
    nd = len(raw)
    dense, k, live, _, _ = ssm.density_rank(nd, density_words, skip, n_bases)
    values = ssm.load_scalars(raw, fmt)
    return sum(v * int(bases[int(ki)]) for v, ki, l in zip(values, k, live) if l)


# ---------------------------------------------------------------------------------------------------------------------------
# the error-resolution pass
# ---------------------------------------------------------------------------------------------------------------------------
def ceil_ln(n):
    """the smallest integer c with e^c >= n, in 60 decimal digits (no integer comes that close to a power of e)"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        c = 0
        while decimal.Decimal(c).exp() < n:
            c += 1
        return c


def lo_ref(nref):
    """first bit of the reference's top window: windows of c = 3 bits below 32 exponents, of ceil(ln n) from there on"""
    c = 3 if nref < 32 else ceil_ln(nref)
    w = (255 + c - 1) // c
    return c * (w - 1)


def err_resolve(raw, fmt, density_words, word_prefix, skip, n_bases, base_is_identity, nref):
    """ident_top: 1 when a dense scalar before the first EOF entry has a bit in [lo_ref, 256) and its base is the identity.
    word_prefix: the words the kernel is given (it does not count them again)"""
    lo = lo_ref(nref)
    values = ssm.load_scalars(raw, fmt)
    for i, s in enumerate(values):
        k = skip + i
        if density_words is not None:
            word = int(density_words[i >> 6])
            if not (word >> (i & 63)) & 1:
                continue
            k = skip + int(word_prefix[i >> 6]) + bin(word & ((1 << (i & 63)) - 1)).count("1")
        if k >= n_bases:
            continue
        if s >> lo and base_is_identity[k]:
            return 1
    return 0
