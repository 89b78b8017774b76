"""The XYZZ group law on RAW projective operands in every lane form, one case per form x operation x tree width (run with
`pytest -m gpu` on a MI355X).

The direct group-law tests of tests/test_gpu_parity.py feed affine points: ZZ = ZZZ = 1 on both sides, canonical
coordinates, P + P only ever bit-identical.  What the merges add is two partial sums with unrelated ZZ and coordinates
anywhere in [0, 2p), and whether they are the same point, opposite points or an identity is decided from is_zero of a
lazily reduced difference - computed, in the lane-pair (K2) and lane-sextet (K6) forms, on one half of the lanes and carried
to the other half by ballot / DPP / shuffle.  Here every operation runs ON ITS OWN through bh_test_group_ops_dev - xyzz_add,
both overloads of xyzz_madd, xyzz_dbl, xyzz_dbl_affine, the conversions, half_add on lane pairs and on lane sextets, the shuffle trees and
long_block_sum, with the kernels' worker and lane mapping - over the tables of tests/group_model.py: every branch class
with its own pair of scalings, interleaved within wavefronts and as whole wavefronts of one branch.  All checks are exact:
  * every returned coordinate < 2p; ZZ^3 = ZZZ^2; (X / ZZ, Y / ZZZ) equals the integer model's affine sum;
  * the result is the identity exactly when the model's is, and the identity flag says so in every lane of the worker;
  * an identity operand gives a bit-exact copy, opposite points the all-zero record, to_affine canonical coordinates;
  * forms 0 and 2: every raw limb equals the host build of the same header;
  * forms 1, 3, 4, 5: the canonicalised coordinates equal the canonicalised host result for the same operands.  No form
    takes a different formula for any operation: K2 / K6 run add-2008-s as seven lane-local product slots with the same
    products and the same ZZ3 = ZZ1 ZZ2 PP, ZZZ3 = ZZZ1 ZZZ2 PPP, and fall back to the one-lane / lane-triple xyzz_dbl;
    the lane-triple and lane-pair forms instantiate the very templates of csrc/ec.cuh.  load_store has no host twin (the
    result must equal the operand bit for bit); to_affine exists for the one-lane forms only (the lane bundles have no
    inversion and no kernel converts in those forms);
  * every table also runs with n = 1, and its full length leaves a ragged last wavefront; guard bytes after the result
    and flag arrays come back untouched (group_model.run_dev).
tests/test_group_model_cpu.py validates the tables and runs the one-lane forms through the host build without a GPU.
Whether and when this file ran on an MI355X: profiles/group_law_gputests.txt."""

import pytest

pytestmark = pytest.mark.gpu

from tests import group_model as gm  # noqa: E402


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


@pytest.mark.parametrize("case", gm.cases(), ids=gm.case_id)
def test_group_operation_on_raw_operands(worker, lib, case):
    form, op, G = case
    name = gm.OPS[op]
    table = gm.operands_for(case)
    assert len(table) == gm.TABLE_SIZES[gm.case_id(case)]
    res, flags = gm.run_dev(lib, worker, form, op, G, table)
    assert gm.check(form, op, G, table, res, flags) == len(table)
    if name != "load_store":
        host_form = 0 if gm.GROUP[form] == 1 else 2
        host_res, host_flags = gm.run_host(lib, host_form, op, gm.TREE_PER_WAVE[form] if name == "block_sum" else G, table)
        assert gm.check_against_host(case, table, res, host_res, exact=form == host_form) == len(table)
        if form == host_form:
            assert (flags == host_flags).all()
    # one worker on its own: a single lane group in the wavefront (a tree: one group, the rest of the wavefront identities)
    for k in (0, len(table) // 2, len(table) - 1):
        res1, flags1 = gm.run_dev(lib, worker, form, op, G, table[k:k + 1])
        assert gm.check(form, op, G, table[k:k + 1], res1, flags1) == 1
        assert res1[0] == res[k] and (flags1[0] == flags[k]).all()
