"""GPU parity of the digit / sort stage of window-table plans (run with `pytest -m gpu` on a MI355X).

A multiexp over bases registered with a window table sorts ONE stream of Wd * n entries (csrc/msm_stages.hip, 2b): the
first pass recodes the scalars itself, a tile being a block of consecutive scalars times all Wd rows, keeps the non-zero
digits only and keys on |d| - 1 in passes of up to 10 bits.  Checked here through the public `multiexp`, against the
restated multiexp of oracle/ (src/multiexp.rs:210-332, error codes included) and, for the counters of
`bh_msm_wait_stats`, against a signed-digit recoding done in Python:

  * G1 with 10-, 13- and 20-bit rows (one pass of 9 bits, 6 + 6, 10 + 9), G2 with 13- and 16-bit rows (6 + 6, 8 + 7); sizes
    that are neither multiples of the first pass's tile nor of 64, one of them exactly one scalar past a tile boundary;
    G1 once with 2-, 5-, 11-, 12-, 21-, 22- and 24-bit rows (one to three passes of 1 to 10 bits);
  * scalars at the key extremes: digits of exactly 2^(c-1) (the largest key), digits 1, carries rippling through every
    row, all zero, and every mix of tests/scalar_mixes.py (`ones`: the whole vector in one bin of every pass);
  * density maps (0.5 and sparse) with a base offset, and a base vector shorter than the dense count (UnexpectedEof);
  * the same job twice: identical result and counters.
Integer work: exact equality of every limb."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cref  # noqa: E402
from tests import scalar_mixes  # noqa: E402

# (group, row bits): Bases.precompute(bits) - the automatic choice differs at these sizes
CONFIGS = [(1, 10), (1, 13), (1, 20), (2, 13), (2, 16)]


def rows(c):
    return (256 + c - 1) // c


def first_pass_tile(c):
    """scalars per tile of the first pass (msm_stages.hip wide_scalars_per_tile: 512 at most, 7168 entries at most)"""
    return max(1, min(512, 7168 // rows(c)))


def nonzero_digits(values, c):
    """how many of the rows(c) signed c-bit digits (low to high with carry, |d| <= 2^(c-1)) of the values are non-zero"""
    half, mask, count = 1 << (c - 1), (1 << c) - 1, 0
    for s in values:
        carry = 0
        for w in range(rows(c)):
            v = ((s >> (w * c)) & mask) + carry
            carry = 0
            if v > half:
                v, carry = (1 << c) - v, 1
            count += v != 0
        assert carry == 0
    return count


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


_HOST_BASES = {}


def host_bases(group, n):
    if group not in _HOST_BASES or _HOST_BASES[group].shape[0] < n:
        _HOST_BASES[group] = cref.gen_bases(group, n, a=7, b=11)
    return _HOST_BASES[group][:n]


def registered(worker, group, c, arr):
    import bellman_amd

    hb = bellman_amd.Bases(worker, group, arr)
    hb.precompute(c)
    assert hb.table_info()[0] == c
    return hb


def run_table(worker, hb, dens, sc, skip=0, mont=False):
    """the table plan through the sort (never the one-launch path of tiny jobs); (record, counters)"""
    import bellman_amd
    from bellman_amd.multiexp import NO_SMALL_PATH

    got, _, st = bellman_amd.multiexp(worker, hb, dens, sc, skip=skip, mont=mont, flags=NO_SMALL_PATH, stats=True).wait()
    assert st["bucket_sets"] == 1 and st["digit_columns"] == rows(st["window_bits"])
    return got, st


def check(worker, group, c, sc, bits=None, skip=0):
    """one job against the oracle and the Python recoding; returns its counters"""
    import bellman_amd

    n = sc.shape[0]
    dense = n if bits is None else int(bits.sum())
    arr = host_bases(group, skip + dense + 3)
    hb = registered(worker, group, c, arr)
    if bits is None:
        dens, dens_c = bellman_amd.FullDensity(), None
    else:
        dens, dens_c = bellman_amd.DensityTracker(), cref.density_bitmap(bits)
        dens.bv = bits
    rc, want = cref.multiexp(group, arr, skip, dens_c, sc)
    assert rc == 0
    got, st = run_table(worker, hb, dens, sc, skip=skip)
    hb.release()
    assert st["window_bits"] == c
    assert np.array_equal(got, want), (group, c, n, skip)
    live = cref.arr_to_ints(sc if bits is None else sc[bits])
    assert st["sorted_entries"] == rows(c) * n
    nonzero = nonzero_digits(live, c)
    # (the counter is reported by the accumulation launch: a job without a single non-zero digit reports none)
    assert st["zero_digits"] == (rows(c) * n - nonzero if nonzero else 0), (group, c, n)
    return st


def extreme_scalars(c, n, seed):
    """n scalars: the patterns that hit the ends of the key range and the carry chain, the rest uniform"""
    W, q = rows(c), cref.Q
    vals = [0, 1, 2, q - 1, q - 2, (1 << 254) - 1, (1 << 254), (1 << 254) + 1]
    # every row's digit exactly 2^(c-1): the largest key of every pass, no carry ...
    vals.append(sum(1 << (c * j + c - 1) for j in range(W - 1)))
    # ... and 2^(c-1) + 1 everywhere: -(2^(c-1) - 1) with a carry into every next row
    vals.append(sum((1 << (c * j + c - 1)) + (1 << (c * j)) for j in range(W - 1)))
    # digit 1 in every row
    vals.append(sum(1 << (c * j) for j in range(W)) % q)
    for j in range(1, W + 1):
        for v in ((1 << (c * j)) - 1, 1 << (c * j - 1), (1 << (c * j - 1)) + 1, (1 << (c * j - 1)) - 1):
            if v < q:
                vals.append(v)
    sc = scalar_mixes.scalars("uniform", n, seed)
    reps = max(1, n // (4 * len(vals)))   # a quarter of the vector, interleaved with the uniform rest
    special = cref.ints_to_arr(vals, 4)
    for r in range(reps):
        at = (np.arange(len(vals)) * reps + r) * 4
        at = at[at < n]
        sc[at] = special[: len(at)]
    return np.ascontiguousarray(sc)


@pytest.mark.parametrize("group,c", CONFIGS)
def test_sizes_around_tile_boundaries(worker, group, c):
    """uniform scalars; sizes: one scalar past a tile boundary of the first pass, one short of it, an odd size in between"""
    spt = first_pass_tile(c)
    k = 8 if group == 1 else 4
    for n in (k * spt + 1, k * spt - 1, (k - 1) * spt + spt // 3 + 1):
        assert n % 64 != 0 and n % spt != 0
        check(worker, group, c, scalar_mixes.scalars("uniform", n, 0x50 + n))


@pytest.mark.parametrize("c", [2, 5, 11, 12, 21, 22, 24])
def test_other_row_widths(worker, c):
    """the ends of what a table can have: 128 rows of 2 bits (one 1-bit pass, 56 scalars per tile), one pass of 4 and of 10
    bits, 6 + 5, 10 + 10, and the three-pass splits 7 + 7 + 7 and 8 + 8 + 7"""
    n = 9 * first_pass_tile(c) + 1
    check(worker, 1, c, scalar_mixes.scalars("uniform", n, 0xC0 + c))
    check(worker, 1, c, extreme_scalars(c, 1201, 0xC1 + c))


def test_g1_20_bit_rows_many_tiles(worker):
    """2 x 10^5 scalars with 20-bit rows: hundreds of tiles in both passes, one scalar past a tile boundary"""
    n = 200 * first_pass_tile(20) + 1
    check(worker, 1, 20, scalar_mixes.scalars("uniform", n, 0x2020))


@pytest.mark.parametrize("group,c", CONFIGS)
def test_key_extremes_and_carries(worker, group, c):
    n = 3001 if group == 1 else 1500
    check(worker, group, c, extreme_scalars(c, n, 0xE0 + c))
    # Montgomery-form scalars take the same recoding
    arr = host_bases(group, n)
    hb = registered(worker, group, c, arr)
    sc = extreme_scalars(c, n, 0xE1 + c)
    rc, want = cref.multiexp(group, arr, 0, None, sc)
    import bellman_amd

    got, _ = run_table(worker, hb, bellman_amd.FullDensity(), cref.fr_to_mont(sc), mont=True)
    hb.release()
    assert rc == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("group,c", CONFIGS)
def test_all_zero_scalars(worker, group, c):
    n = 2 * first_pass_tile(c) + 5
    check(worker, group, c, np.zeros((n, 4), dtype=np.uint64))


@pytest.mark.parametrize("mix", scalar_mixes.MIXES)
@pytest.mark.parametrize("group,c", CONFIGS)
def test_scalar_mixes(worker, group, c, mix):
    n = 5 * first_pass_tile(c) + 77 if group == 1 else 2 * first_pass_tile(c) + 77
    check(worker, group, c, scalar_mixes.scalars(mix, n, 0x31C + c))


@pytest.mark.parametrize("p", [0.5, 0.02])
@pytest.mark.parametrize("group,c", CONFIGS)
def test_density_maps_with_skip(worker, group, c, p):
    n = 6 * first_pass_tile(c) + 13 if group == 1 else 3 * first_pass_tile(c) + 13
    rnd = np.random.default_rng(0xDE + c + group)
    bits = rnd.random(n) < p
    bits[-1] = True
    check(worker, group, c, scalar_mixes.scalars("bool50", n, 0xD5 + c), bits=bits, skip=5)


@pytest.mark.parametrize("group,c", CONFIGS)
def test_short_base_vector_is_eof(worker, group, c):
    """fewer bases than dense entries: UnexpectedEof, as the oracle and the classic plan report it"""
    import bellman_amd
    from bellman_amd import UnexpectedEof
    from bellman_amd.multiexp import NO_TABLE

    n = 3 * first_pass_tile(c) + 2
    sc = scalar_mixes.scalars("uniform", n, 0xE0F + c)
    sc[-1] = 0   # the entry past the end has a zero scalar: EOF all the same
    rnd = np.random.default_rng(0xE0F)
    bits = rnd.random(n) < 0.5
    bits[-1] = True
    dens = bellman_amd.DensityTracker()
    dens.bv = bits
    for d, d_c, count in ((bellman_amd.FullDensity(), None, n), (dens, cref.density_bitmap(bits), int(bits.sum()))):
        arr = host_bases(group, 4 + count - 1)   # one base short after skip = 4
        rc, _ = cref.multiexp(group, arr, 4, d_c, sc)
        assert rc == 2
        hb = registered(worker, group, c, arr)
        with pytest.raises(UnexpectedEof):
            run_table(worker, hb, d, sc, skip=4)
        with pytest.raises(UnexpectedEof):
            bellman_amd.multiexp(worker, hb, d, sc, skip=4, flags=NO_TABLE).wait()
        hb.release()


@pytest.mark.parametrize("group,c", [(1, 20), (1, 10), (2, 16)])
def test_same_job_twice_is_identical(worker, group, c):
    import bellman_amd

    n = 7 * first_pass_tile(c) + 3 if group == 1 else 2 * first_pass_tile(c) + 3
    sc = scalar_mixes.scalars("small90", n, 0x7E)
    hb = registered(worker, group, c, host_bases(group, n))
    a, sa = run_table(worker, hb, bellman_amd.FullDensity(), sc)
    b, sb = run_table(worker, hb, bellman_amd.FullDensity(), sc)
    hb.release()
    assert np.array_equal(a, b) and sa == sb
