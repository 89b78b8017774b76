"""Integer model of stages 1 - 3 of a multiexp (csrc/msm_stages.hip, csrc/msm_scalar.cuh): scalar load, density rank, signed
digit recoding, and the sorted pair stream of the classic plan (every window stable by |digit|) and of the table plan (live
non-zero digits only, key |d| - 1, inside a key by scalar block, wavefront, row, scalar).  numpy where a Python loop would be
slow; nothing here calls the library - the tile sizes are arguments."""
import numpy as np

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R_INV = pow(1 << 256, -1, Q)
WAVE = 64


def windows(c):
    return (256 + c - 1) // c


def load_scalars(raw, fmt):
    """what load_scalar leaves in registers: canonical values below 2^256 minus q at most twice, Montgomery values (below q)
    times R^-1"""
    out = []
    for v in raw:
        assert 0 <= v < (1 << 256)
        if fmt == 1:
            assert v < Q
            v = v * R_INV % Q
        else:
            for _ in range(2):
                if v >= Q:
                    v -= Q
        out.append(v)
    return out


def to_words(values):
    """-> uint32 [n][8], little endian"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u4").reshape(-1, 8).copy()


def density_rank(nd, density_words, skip, n_bases):
    """-> (dense, k, live, eof, word_prefix or None).  k = skip + dense bits before i; live = dense and k < n_bases; eof when a
    dense scalar has k >= n_bases, whatever its value"""
    if density_words is None:
        dense = np.ones(nd, dtype=bool)
        prefix = None
        k = skip + np.arange(nd, dtype=np.uint64)
    else:
        words = np.asarray(density_words, dtype=np.uint64)
        assert len(words) == (nd + 63) // 64
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        pop = bits.reshape(-1, 64).sum(axis=1)
        prefix = (np.cumsum(pop) - pop).astype(np.uint32)   # over ALL bits of a word, those past nd included
        dense = bits[:nd].astype(bool)
        before = np.cumsum(bits[:nd], dtype=np.uint64) - bits[:nd]
        k = skip + before
    live = dense & (k < n_bases)
    eof = bool((dense & (k >= n_bases)).any())
    return dense, k.astype(np.uint64), live, eof, prefix


def recode(values, c):
    """signed digits, low to high with carry: -> (|d| uint32 [n][W], sign uint32 [n][W], carry out of the top digit [n])"""
    W = windows(c)
    n = len(values)
    words = np.zeros((n, 10), dtype=np.uint64)
    if n:
        words[:, :8] = to_words(values)
    half = np.uint64(1 << (c - 1))
    mag = np.zeros((n, W), dtype=np.uint32)
    sign = np.zeros((n, W), dtype=np.uint32)
    carry = np.zeros(n, dtype=np.uint64)
    for w in range(W):
        lo = w * c
        two = words[:, lo >> 5] | (words[:, (lo >> 5) + 1] << np.uint64(32))
        v = ((two >> np.uint64(lo & 31)) & np.uint64((1 << c) - 1)) + carry
        neg = v > half
        v = np.where(neg, np.uint64(1 << c) - v, v)
        mag[:, w] = v
        sign[:, w] = neg & (v != 0)       # 2^c - v == 0: digit 0 with a carry out, sign clear
        carry = neg.astype(np.uint64)
    return mag, sign, carry


def entries(mag, sign, k, stride):
    """[n][W] entry words: |d| << 32 | sign << 31 | ((k + w * stride) & 0x7fffffff)"""
    W = mag.shape[1]
    base = (k[:, None] + np.arange(W, dtype=np.uint64)[None, :] * np.uint64(stride)) & np.uint64(0x7FFFFFFF)
    return (mag.astype(np.uint64) << np.uint64(32)) | (sign.astype(np.uint64) << np.uint64(31)) | base


def stage(kind, c, raw, fmt, density_words, skip, n_bases, stride, spt=None):
    """-> dict: zstart, eof, word_prefix, live (entries of the table stream), passes: the key masks after which the classic
    plan's arrays are defined, and

    classic  result [W][n] (every window stable by |d|), after(p) = the [W][n] array after p passes (p = 0: unsorted)
    table    stream (the sorted live non-zero entries; it occupies [zstart, n) of the result array), after(p) = the live
             entries after p passes
    """
    nd = len(raw)
    W = windows(c)
    dense, k, live, eof, prefix = density_rank(nd, density_words, skip, n_bases)
    values = load_scalars(raw, fmt)
    values = [v if l else 0 for v, l in zip(values, live)]   # a scalar that is not live is never loaded: digit 0 everywhere
    mag, sign, carry = recode(values, c)
    assert not carry.any(), "the top digit of a reduced scalar has no carry out"
    e = entries(mag, sign, k, stride)
    out = dict(eof=int(eof), word_prefix=prefix, c=c, W=W, nd=nd, kind=kind)
    if kind == 0:
        assert stride == 0
        unsorted = np.ascontiguousarray(e.T)                 # window-major
        digits = np.ascontiguousarray(mag.T)

        def after(p):
            if p == 0:
                return unsorted
            key = digits & np.uint32((1 << (8 * p)) - 1)
            order = np.argsort(key, axis=1, kind="stable")
            return np.take_along_axis(unsorted, order, axis=1)

        passes = (c + 7) // 8
        out.update(after=after, passes=passes, result=after(passes), zstart=(digits == 0).sum(axis=1).astype(np.uint32))
        return out
    assert spt
    i = np.repeat(np.arange(nd, dtype=np.int64), W).reshape(nd, W)
    w = np.tile(np.arange(W, dtype=np.int64), nd).reshape(nd, W)
    keep = live[:, None] & (mag != 0)
    ek, ik, wk = e[keep], i[keep], w[keep]
    key = (ek >> np.uint64(32)).astype(np.int64) - 1
    nlive = int(keep.sum())

    def after(bits):
        """the live entries once the low `bits` key bits are sorted"""
        low = key & ((1 << bits) - 1)
        order = np.lexsort((ik, wk, (ik % spt) // WAVE, ik // spt, low))
        return ek[order]

    out.update(after=after, live=nlive, stream=after(c - 1), zstart=np.array([W * nd - nlive], dtype=np.uint32))
    return out


def table_pass_bits(c, max_bits=10):
    """key bits per pass: c - 1 bits in ceil((c - 1) / 10) passes, split evenly, the remainder to the FIRST passes"""
    kb = c - 1
    np_ = (kb + max_bits - 1) // max_bits
    return [kb // np_ + (1 if p < kb % np_ else 0) for p in range(np_)]


def stream_ok(stream, c, n_rows_records):
    """the conditions the bucket-stage hook puts on a stream: keys non-decreasing in [1, 2^(c-1)], base fields inside the table"""
    d = (stream >> np.uint64(32)).astype(np.int64)
    idx = (stream & np.uint64(0x7FFFFFFF)).astype(np.int64)
    return bool((d >= 1).all() and (d <= (1 << (c - 1))).all() and (np.diff(d) >= 0).all() and (idx < n_rows_records).all())


def scan_layout(n, tile):
    """the accesses of exclusive_scan_u32 to its scratch: -> (largest index touched + 1, [(offset, slots) per level])"""
    levels, off, top = [], 0, 0
    while True:
        blocks = (n + tile - 1) // tile
        levels.append((off, blocks))       # scan_tile_kernel writes one slot per tile at `off`
        top = max(top, off + blocks)
        if blocks <= 1:
            break
        off += (blocks + 63) & ~63         # the next level's scratch starts at the count rounded up to 64
        n = blocks
    return top, levels


def exclusive_scan(data):
    data = np.asarray(data, dtype=np.uint64)
    out = np.cumsum(data) - data
    assert len(data) == 0 or int(out[-1] + data[-1]) < (1 << 32)
    return out.astype(np.uint32)


def scan_scratch(data, tile, tmp_elems, sentinel_word):
    """what the scratch holds after the scan: per level the exclusive scan of the level's tile sums - the last level's single
    slot holds the grand total - and the sentinel everywhere else"""
    tmp = np.full(tmp_elems, sentinel_word, dtype=np.uint32)
    cur, off = np.asarray(data, dtype=np.uint64), 0
    while True:
        sums = np.add.reduceat(cur, np.arange(0, len(cur), tile))
        if len(sums) == 1:
            tmp[off] = sums[0]
            return tmp
        tmp[off:off + len(sums)] = exclusive_scan(sums)
        off += (len(sums) + 63) & ~63
        cur = sums
