"""Device field arithmetic at corner operands, one case per form x operation (run with `pytest -m gpu` on a MI355X).

Every result of the library is a chain of Fp, Fp2 and Fp12 operations; in a whole MSM, group law or pairing their operands
are random curve data, which sit in the middle of every range.  Here each operation runs ON ITS OWN through
bh_test_field_ops_dev - the function objects the kernels call (FpOps, Fp2Ops, Fp2K3Ops, Fp2PairOps with the kernels' lane
mapping, the tower of csrc/fp12.cuh, the square roots of csrc/point_read.cuh) - over the tables of tests/field_model.py:
both representatives of zero, operands at 2p - 1, limbs at their maximum, sums that land exactly on 2p, fused products
whose subtrahend is zero (the multiplier is then fed 2p).  No tolerances:
  * canonical forms: every limb equals the integer result;
  * lazily reduced forms: congruent to the integer result mod p AND within the bound the code documents
    (add / sub / neg / dbl < 2p; product < a b / 2^384 + p + 1; fused product < (a b + (2p - c) d) / 2^384 + p + 1;
    neg(0) = 0; canon exact);
  * device against host: every raw limb equals the host build of the same header (the representative is deterministic);
  * predicates: the flags equal x = 0 / a = b mod p, the same in every lane of a lane group;
  * square roots: ok equals the Euler criterion (the norm test in Fp2), r^2 = a when it is set.
tests/test_field_model_cpu.py runs the same tables through the host build and pins the table sizes."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import field_model as fm  # noqa: E402

# lane forms: the operations whose lanes hold, by construction, the very representative the one-lane Fp2Ops computes
# (lane-local fpl_* calls; the triple's product recombines as t0 - t1 and (t2 - t0) - t1 like Fp2Ops::mul) - the c0 / c1
# lanes are then compared bit for bit with the host build of Fp2Ops.  The pair product (schoolbook, fused) and both
# squarings take other routes to the same value: congruence and bounds only - for the pair form the multiplier's own bound,
# since each of its lanes holds one (fused) Montgomery product (field_model._check_lanes).
LANES_SAME_AS_ONE_LANE = {4: ("add", "sub", "neg", "dbl", "canon", "mul"), 5: ("add", "sub", "neg", "dbl", "canon")}


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("case", fm.cases(), ids=fm.case_id)
def test_field_operation_at_corner_operands(worker, lib, case):
    form, op = case
    operands = fm.operands_for(case)
    assert len(operands) == fm.TABLE_SIZES[fm.case_id(case)]
    raw, flags = fm.run_dev(lib, worker, form, op, operands)
    assert fm.check(form, op, operands, raw, flags) == len(operands)
    if form in (4, 5):
        name = fm.LANE_OPS[op]
        if name in LANES_SAME_AS_ONE_LANE[form]:
            host_op = {v: k for k, v in fm.LAZY_OPS.items()}[name]
            host_raw, _ = fm.run_host(lib, 3, host_op, operands)
            assert np.array_equal(raw[1], host_raw), _first_difference(case, operands, raw[1], host_raw)
        # one element on its own: a single lane group in the wavefront
        for e in (operands[0], operands[len(operands) // 2]):
            raw1, flags1 = fm.run_dev(lib, worker, form, op, [e])
            assert fm.check(form, op, [e], raw1, flags1) == 1
    else:
        host_raw, host_flags = fm.run_host(lib, form, op, operands)
        assert np.array_equal(raw, host_raw), _first_difference(case, operands, raw, host_raw)
        assert np.array_equal(flags, host_flags)


def _first_difference(case, operands, dev, host):
    i = int(np.nonzero((dev != host).any(axis=1))[0][0])
    return "%s: element %d %r: device %s, host %s" % (fm.case_id(case), i, [hex(v) for v in fm.flat(operands[i])],
                                                      [hex(v) for v in fm.unpack(dev[i:i + 1])[0]],
                                                      [hex(v) for v in fm.unpack(host[i:i + 1])[0]])


def test_field_hook_leaves_what_lies_beyond_n_alone(worker, lib):
    """the lane kernels write n * LANES lane values and n stored values and nothing after them (ragged last wavefront)"""
    for form, lanes in ((4, 3), (5, 2)):
        ops = fm.operands_for((form, 7))[:50]
        n = len(ops)
        _, _, arrs = fm.operand_arrays(lib, form, 7, ops)
        da, db = worker.alloc(arrs[0].nbytes), worker.alloc(arrs[1].nbytes)
        worker.upload(da, arrs[0])
        worker.upload(db, arrs[1])
        guard = 4096
        out = np.full(n * (lanes * 48 + 96) + guard, 0xA5, dtype=np.uint8)
        fl = np.full(n * lanes + 64, 0xA5A5A5A5, dtype=np.uint32)
        do, df = worker.alloc(out.nbytes), worker.alloc(fl.nbytes)
        worker.upload(do, out)
        worker.upload(df, fl)
        assert lib.bh_test_field_ops_dev(worker.ctx, form, 7, do, df, da, db, None, None, n) == 0
        worker.download(out, do)
        worker.download(fl, df)
        for d in (da, db, do, df):
            worker.free(d)
        assert (out[-guard:] == 0xA5).all() and (fl[n * lanes:] == 0xA5A5A5A5).all() and not fl[:n * lanes].any()
