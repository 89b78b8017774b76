"""Which of a base handle's sources a multiexp reads: msm_pick_sources (csrc/msm_types.hpp) through bh_test_msm_sources
against its rule table, written out here, over the full product of its inputs.  No GPU: the hook hands the picker views
whose pointers are tags.

  use_table        a table is present, no BH_MSM_NO_TABLE, window_bits is 0 or the table's, rows x records per row
                   < 2^31 and rows x scalars < 2^32
  gather           table plan: the table at its stride; classic plan: the 128-byte-stride copy if there is one and the
                   job is G1 with one lane per point and the accumulator in registers, else the registered vector
  error resolution the table if use_table (row 0 is a snapshot of the bases), else the registered vector
  small path       use_table and the table sits at the dense record stride (msm_small_fill_kernel indexes Affine<M> *)
"""
import ctypes
import itertools

import pytest

from bellman_amd.multiexp import ACC_LDS, NO_TABLE

INVALID_ARG = -2                                 # BH_ERR_INVALID_ARG
DENSE, PADDED, TABLE = 0, 1, 2                   # the views, as the hook names them
REGISTERS, LDS, MULTI_LANE = 0, 1, 2             # accumulate forms
TAB_C, TAB_W = 16, 16                            # 16 rows of 16 bits: the limits are hit exactly
# (records per table row, scalars): small; rows x records just below and at 2^31; rows x scalars just below and at 2^32
SIZES = [(1024, 1024), ((1 << 27) - 1, 1024), (1 << 27, 1024), (1024, (1 << 28) - 1), (1024, 1 << 28)]


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load().test


def pick(lib, group, kind, padded, flags, opts_c, row, n, form):
    out = (ctypes.c_uint32 * 6)()
    rc = lib.bh_test_msm_sources(group, kind, padded, flags, opts_c, TAB_C, TAB_W, row, n, form, out)
    return rc, [int(v) for v in out]


def test_hook_refuses_what_does_not_exist(lib):
    assert pick(lib, 3, 0, 0, 0, 0, 1024, 1024, 0)[0] == INVALID_ARG       # no such group
    assert pick(lib, 1, 3, 0, 0, 0, 1024, 1024, 0)[0] == INVALID_ARG       # no such table layout
    assert pick(lib, 1, 0, 0, 0, 0, 1024, 1024, 3)[0] == INVALID_ARG       # no such accumulate form


def test_sources_follow_the_rule_table_over_the_full_product(lib):
    seen = set()
    for group, kind, padded, no_table, c_sel, form, (row, n) in itertools.product(
            (1, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1, 2), (REGISTERS, LDS, MULTI_LANE), SIZES):
        opts_c = (0, TAB_C, TAB_C + 1)[c_sel]
        # (ACC_LDS rides along where the form is the LDS one, as in a real job: the picker must not look at it)
        flags = (NO_TABLE if no_table else 0) | (ACC_LDS if form == LDS else 0)
        rec = 96 if group == 1 else 192
        rc, (use, g_view, g_stride, r_view, r_stride, small) = pick(lib, group, kind, padded, flags, opts_c, row, n, form)
        case = (group, kind, padded, no_table, opts_c, form, row, n)
        if group == 2 and kind == 2:
            assert rc == INVALID_ARG, case           # only G1 tables are laid out at a 128-byte stride
            continue
        assert rc == 0, case
        t_stride = 128 if kind == 2 else rec
        want_use = kind != 0 and not no_table and opts_c in (0, TAB_C) and TAB_W * row < 1 << 31 and TAB_W * n < 1 << 32
        if want_use:
            want_gather = want_resolve = (TABLE, t_stride)
        else:
            want_gather = (PADDED, 128) if padded and group == 1 and form == REGISTERS else (DENSE, rec)
            want_resolve = (DENSE, rec)
        assert use == int(want_use), case
        assert (g_view, g_stride) == want_gather, case
        assert (r_view, r_stride) == want_resolve, case
        assert small == int(want_use and t_stride == rec), case
        # what the kernels rely on
        assert not (small and g_stride != rec), case
        assert not (group == 2 and 128 in (g_stride, r_stride)), case
        seen.add((use, g_view, g_stride, r_view, small))
    # every outcome the table names was reached
    assert {(1, TABLE, 128, TABLE, 0), (1, TABLE, 96, TABLE, 1), (1, TABLE, 192, TABLE, 1), (0, PADDED, 128, DENSE, 0),
            (0, DENSE, 96, DENSE, 0), (0, DENSE, 192, DENSE, 0)} == seen
