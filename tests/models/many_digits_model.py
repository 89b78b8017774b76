"""Plain-Python restatement of the digit stage of a many-plan (csrc/msm_stages.hip, msm_many_digits_kernel): k scalar
vectors over ONE base vector and density map, written so that every bucket set is a contiguous region of pairs.

A pair is |digit| << 32 | sign << 31 | base field.  With nd scalars per vector, Wd = ceil(256 / c) digit columns:

  digit j of scalar i of vector v sits at   pairs[(v * Wd + j) * nd + i]
  classic flavour (base_stride = 0)         bucket set v * Wd + j, position i,          base field = skip + rank_i
  table flavour   (base_stride = row len)   bucket set v,          position j * nd + i, base field = skip + rank_i + j * stride

rank_i = number of dense entries before i (i itself when there is no density map).  A scalar that is not dense, or whose
base index is at or beyond n_bases (which also raises the job's EOF flag), contributes zero digits."""

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def signed_digits(s, c):
    """ceil(256 / c) signed c-bit digits of s < 2^255, low to high with carry: (|d|, negative) per column;
    sum d_j 2^(c j) == s and |d_j| <= 2^(c-1)"""
    wd = (256 + c - 1) // c
    half = 1 << (c - 1)
    out, carry = [], 0
    for j in range(wd):
        v = ((s >> (c * j)) & ((1 << c) - 1)) + carry
        carry, neg = 0, 0
        if v > half:
            v = (1 << c) - v
            neg = 1 if v else 0
            carry = 1
        out.append((v, neg))
    assert carry == 0
    return out


def base_indices(nd, density, skip):
    """(dense_i, skip + rank_i) per scalar index"""
    out, rank = [], 0
    for i in range(nd):
        d = True if density is None else bool(density[i])
        out.append((d, skip + rank))
        rank += 1 if d else 0
    return out


def many_pairs(vectors, c, density=None, skip=0, n_bases=None, base_stride=0):
    """vectors: k lists of nd integers (already reduced mod q).  Returns (pairs, eof): the flat list of k * Wd * nd
    pairs in the layout above, and whether a dense entry found its base index at or beyond n_bases."""
    k, nd = len(vectors), len(vectors[0])
    wd = (256 + c - 1) // c
    n_bases = skip + nd if n_bases is None else n_bases
    idx = base_indices(nd, density, skip)
    eof = any(d and b >= n_bases for d, b in idx)
    pairs = [0] * (k * wd * nd)
    for v in range(k):
        for i in range(nd):
            dense, b = idx[i]
            live = dense and b < n_bases
            digs = signed_digits(vectors[v][i] % Q if live else 0, c)
            for j, (mag, neg) in enumerate(digs):
                base = (b + j * base_stride) & 0xFFFFFFFF & 0x7FFFFFFF
                pairs[(v * wd + j) * nd + i] = (mag << 32) | (neg << 31) | base
    return pairs, eof


def bucket_sets(pairs, k, nd, c, table):
    """the pairs of every bucket set as a list of lists: k sets of Wd * nd pairs (table flavour) or k * Wd of nd"""
    wd = (256 + c - 1) // c
    per = wd * nd if table else nd
    sets = k if table else k * wd
    return [pairs[s * per:(s + 1) * per] for s in range(sets)]


def zero_counts(sets):
    """zstart per set: how many of its pairs carry digit 0 (they sort to the front and are skipped)"""
    return [sum(1 for e in s if (e >> 32) == 0) for s in sets]
