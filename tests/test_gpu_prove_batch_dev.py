"""The batch prover over witnesses that are in device memory already (bh_groth16_prove_witness_batch_dev,
prove_witness_batch_dev): every proof is prove_witness_batch's on host copies of the same witnesses, byte for byte, with
the tails finished on the host and on the device; the caller's buffers - padding between the vectors included - are
unchanged afterwards; with a check the unsatisfied witnesses get code 11, zero slots and the constraint the integer model
names (tests/models/r1cs_many_model.py); and solve -> check -> prove runs from device buffers that hold only ONE and the
supplied values.  k = 17 crosses the 16 proofs in flight.  The test twin (bh_test_groth16_prove_witness_batch_dev_mode) gives the
same proofs in mode 0 and in mode 3 - the grouped path over the caller's pointers and strides - with one group, with ragged
groups under a small budget, and with an unsatisfied witness in the middle of what would be a group."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import circuits
from tests.models import r1cs_many_model as model
from tests.test_gpu_prove_batch_checked import _corrupt, _setup
from tests.test_gpu_prove_batch_h import _equal
from tests.test_gpu_r1cs_solve import BOOLMIX, MIMC, _demo, _params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = circuits.Q
UNSATISFIABLE = 11
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module", params=["mimc20", "chain61"])
def setup(worker, request):
    """-> (r1cs, params, model system, 17 true witnesses as Montgomery arrays, r, s, prove_witness_batch's proofs): the
    reference proofs are computed once per circuit"""
    from bellman_amd import groth16 as pg
    from bellman_amd.groth16 import fr_to_mont_array

    k = 17
    r1cs, pp, system, wits = _setup(worker, request.param, k)
    rnd = random.Random(77)
    rs, ss = [rnd.randrange(Q) for _ in range(k)], [rnd.randrange(Q) for _ in range(k)]
    ins = np.ascontiguousarray(np.stack([fr_to_mont_array(list(w[0])) for w in wits]))
    auxs = np.ascontiguousarray(np.stack([fr_to_mont_array(list(w[1])) for w in wits]))
    want = pg.prove_witness_batch(r1cs, pp, ins, auxs, rs, ss)
    return r1cs, pp, system, wits, ins, auxs, rs, ss, want


@pytest.mark.parametrize("k", [1, 5, 17])
@pytest.mark.parametrize("stride_extra", [0, 96])
def test_proofs_equal_the_host_entrys_and_the_buffers_are_unchanged(worker, setup, k, stride_extra):
    from bellman_amd import groth16 as pg

    r1cs, pp, _, _, ins, auxs, rs, ss, want = setup
    dw = pg.DeviceWitnesses.from_host(worker, ins[:k], auxs[:k], stride_extra)
    before = dw.download_raw()
    for finish in ("host", "device", None):
        got = pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], finish=finish)
        assert len(got) == k and all(_equal(got[j], want[j]) for j in range(k)), finish
    after = dw.download_raw()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])   # vectors and padding
    if stride_extra:
        assert (after[1][:, -stride_extra // 8:] == 0x5A5A5A5A5A5A5A5A).all()
    dw.release()


def _ragged_budget(r1cs, g):
    """a workspace budget under which the grouped path's groups hold g witnesses: 4 * g * m * 32 bytes"""
    m = 1
    while m < r1cs.num_constraints:
        m *= 2
    return 4 * g * m * 32


@pytest.mark.parametrize("k", [1, 5, 17])
@pytest.mark.parametrize("stride_extra", [0, 96])
def test_twin_modes_0_and_3_equal_the_host_entry(worker, setup, k, stride_extra):
    """the test twin: mode 0 (the call as shipped) and mode 3 (BATCH_GROUPED_HE over the caller's pointers and strides) with
    one group, and mode 3 under a budget of 3 witnesses per group - 17 = 3 x 5 + 2, 5 = 3 + 2: ragged groups"""
    from bellman_amd import groth16 as pg

    r1cs, pp, _, _, ins, auxs, rs, ss, want = setup
    dw = pg.DeviceWitnesses.from_host(worker, ins[:k], auxs[:k], stride_extra)
    before = dw.download_raw()
    for mode, budget, finish in ((0, None, "host"), (0, None, "device"), (3, None, "host"), (3, None, "device"),
                                 (3, _ragged_budget(r1cs, 3), "host"), (3, _ragged_budget(r1cs, 3), "device")):
        got = pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], finish=finish, _mode=mode, _workspace_budget=budget)
        assert len(got) == k and all(_equal(got[j], want[j]) for j in range(k)), (mode, budget, finish)
    after = dw.download_raw()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])   # vectors and padding
    dw.release()


@pytest.mark.parametrize("budget_witnesses", [None, 4])
def test_mode_3_with_a_bad_witness_in_the_middle_of_a_group(worker, setup, budget_witnesses):
    """7 witnesses, number 2 and number 6 unsatisfied: under a check the groups are the runs of satisfied witnesses
    [0, 1], [3, 4, 5] (one group of 7 would otherwise hold them all; with 4 per group, number 2 sits inside the first) -
    codes, zero slots and first_unsatisfied as the host entry's, the other proofs prove_witness_batch's"""
    from bellman_amd import groth16 as pg
    from bellman_amd.groth16 import fr_to_mont_array

    r1cs, pp, system, wits, _, _, rs, ss, want = setup
    k = 7
    wits = [(list(w[0]), list(w[1])) for w in wits[:k]]
    wits[2] = _corrupt(wits[2], system.n_aux // 2)
    wits[6] = _corrupt(wits[6], system.n_aux - 1)
    want_first = [model.first_bad(system, w_in, w_aux) for w_in, w_aux in wits]
    assert [w is None for w in want_first] == [True, True, False, True, True, True, False]
    ins = np.ascontiguousarray(np.stack([fr_to_mont_array(w[0]) for w in wits]))
    auxs = np.ascontiguousarray(np.stack([fr_to_mont_array(w[1]) for w in wits]))
    dw = pg.DeviceWitnesses.from_host(worker, ins, auxs, 96)
    budget = None if budget_witnesses is None else _ragged_budget(r1cs, budget_witnesses)
    for finish in ("host", "device"):
        codes, reported = [], []
        got = pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], check=True, finish=finish, _mode=3, _workspace_budget=budget,
                                         _codes=codes, _first_unsatisfied=reported)
        assert codes == [0, 0, UNSATISFIABLE, 0, 0, 0, UNSATISFIABLE] and reported == want_first
        for j in range(k):
            assert (got[j] is None) if codes[j] else _equal(got[j], want[j])
    # without the check the corrupted witnesses are proved as they stand, in one run of 7: prove_witness_batch's proofs of them
    host = pg.prove_witness_batch(r1cs, pp, ins, auxs, rs[:k], ss[:k])
    got = pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], finish="device", _mode=3, _workspace_budget=budget)
    assert all(_equal(got[j], host[j]) for j in range(k))
    dw.release()


@pytest.mark.parametrize("finish", ["host", "device"])
def test_checked_call_names_unsatisfied_witnesses_and_proves_the_rest(worker, setup, finish):
    import bellman_amd
    from bellman_amd import groth16 as pg
    from bellman_amd.groth16 import fr_to_mont_array

    r1cs, pp, system, wits, _, _, rs, ss, want = setup
    k = 5
    wits = [(list(w[0]), list(w[1])) for w in wits[:k]]
    rnd = random.Random(9)
    for j, pos in ((0, rnd.randrange(system.n_aux)), (2, system.n_aux - 1), (4, 0)):   # the first, a middle, the last index
        wits[j] = _corrupt(wits[j], pos)
    want_first = [model.first_bad(system, w_in, w_aux) for w_in, w_aux in wits]
    assert [w is None for w in want_first] == [False, True, False, True, False]
    ins = np.ascontiguousarray(np.stack([fr_to_mont_array(w[0]) for w in wits]))
    auxs = np.ascontiguousarray(np.stack([fr_to_mont_array(w[1]) for w in wits]))
    dw = pg.DeviceWitnesses.from_host(worker, ins, auxs, 96)
    # the C entry itself, every output pre-filled
    lib = bellman_amd._lib.load()
    rr, sv = fr_to_mont_array(rs[:k]), fr_to_mont_array(ss[:k])
    out = np.full((k, 48), SENTINEL, dtype=np.uint64)
    rcs = np.full(k, -77, dtype=np.int32)
    first = np.full(k, 12345, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    flags = pg.PROVE_CHECK | (pg.PROVE_FINISH_DEVICE if finish == "device" else pg.PROVE_FINISH_HOST)
    assert lib.bh_groth16_prove_witness_batch_dev(pp._h, r1cs._h, dw.inputs, dw.in_stride, dw.aux, dw.aux_stride, k, p(rr), p(sv), flags,
                                                  None, p(out), p(rcs), p(first), None) == 0
    assert list(rcs) == [UNSATISFIABLE, 0, UNSATISFIABLE, 0, UNSATISFIABLE]
    assert [None if int(b) == 0xFFFFFFFF else int(b) for b in first] == want_first
    for j in range(k):
        if rcs[j]:
            assert not out[j].any()
        else:
            assert _equal(pg.Proof(out[j].copy()), want[j])
    # exactly the host entry's answers on host copies of the same witnesses
    codes, reported = [], []
    host = pg.prove_witness_batch(r1cs, pp, ins, auxs, rs[:k], ss[:k], check=True, _codes=codes, _first_unsatisfied=reported)
    assert codes == list(rcs) and reported == want_first and [h is None for h in host] == [c != 0 for c in codes]
    # without the check bit first_unsatisfied is untouched and every witness is proved as it stands
    first[:] = 12345
    assert lib.bh_groth16_prove_witness_batch_dev(pp._h, r1cs._h, dw.inputs, dw.in_stride, dw.aux, dw.aux_stride, k, p(rr), p(sv),
                                                  flags & ~pg.PROVE_CHECK, None, p(out), p(rcs), p(first), None) == 0
    assert (first == 12345).all() and not rcs.any() and _equal(pg.Proof(out[1].copy()), want[1])
    with pytest.raises(bellman_amd.Unsatisfiable) as e:
        pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], check=True, finish=finish)
    assert e.value.index == want_first[0]
    dw.release()


def test_refusals_before_anything_runs(worker, setup):
    import bellman_amd
    from bellman_amd import groth16 as pg
    from bellman_amd.groth16 import fr_to_mont_array

    r1cs, pp, _, _, ins, auxs, rs, ss, _ = setup
    k = 2
    dw = pg.DeviceWitnesses.from_host(worker, ins[:k], auxs[:k], 32)
    lib = bellman_amd._lib.load()
    rr, sv = fr_to_mont_array(rs[:k]), fr_to_mont_array(ss[:k])
    out = np.full((k, 48), SENTINEL, dtype=np.uint64)
    rcs = np.full(k, -77, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(in_stride, aux_stride, flags):
        return lib.bh_groth16_prove_witness_batch_dev(pp._h, r1cs._h, dw.inputs, in_stride, dw.aux, aux_stride, k, p(rr), p(sv), flags, None,
                                                      p(out), p(rcs), None, None)

    assert call(dw.in_stride, dw.aux_stride, pg.PROVE_FINISH_DEVICE | pg.PROVE_FINISH_HOST) == -2   # both finish bits
    assert call(dw.in_stride + 8, dw.aux_stride, 0) == -2                                            # not a multiple of 32
    assert call(dw.in_stride, dw.aux_stride - 16, 0) == -2
    assert call(dw.in_stride, r1cs.num_aux * 32 - 32, 0) == -2                                       # shorter than the vector
    assert (out == SENTINEL).all() and (rcs == -77).all()
    with pytest.raises(ValueError):
        pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:k], ss[:k], finish="both")
    with pytest.raises(ValueError):
        pg.prove_witness_batch_dev(r1cs, pp, dw, rs[:1], ss[:k])
    for mode in (1, 2, 4):   # the twin takes modes 0 and 3 alone
        assert lib.bh_test_groth16_prove_witness_batch_dev_mode(pp._h, r1cs._h, dw.inputs, dw.in_stride, dw.aux, dw.aux_stride, k, p(rr),
                                                                p(sv), 0, None, p(out), p(rcs), None, None, 0, mode) == -2
    assert (out == SENTINEL).all() and (rcs == -77).all()
    assert pg.prove_witness_batch_dev(r1cs, pp, pg.DeviceWitnesses.from_host(worker, ins[:0], auxs[:0]), [], []) == []
    dw.release()


@pytest.mark.parametrize("kind,size", [(MIMC, 322), (BOOLMIX, 64)])
def test_solve_check_prove_from_supplied_values_only(worker, kind, size):
    """device buffers that hold nothing but ONE and the supplied values: Solver.solve_many_dev, the check and the prover
    on them - no host copy of a solved witness exists here"""
    import bellman_amd
    from bellman_amd import groth16 as pg

    k = 3
    r1cs, solver, full, supplied = _demo(worker, kind, size, k)
    n_in = r1cs.num_inputs
    params = _params(worker, r1cs)
    rs, ss = [11, 22, 33], [44, 55, 66]
    want = pg.prove_witness_batch(r1cs, params, np.ascontiguousarray(full[:, :n_in]), np.ascontiguousarray(full[:, n_in:]), rs, ss)
    bare = np.zeros_like(full)
    bare[:, [0] + supplied] = full[:, [0] + supplied]
    for finish in ("device", "host"):
        dw = pg.DeviceWitnesses.from_host(worker, bare[:, :n_in], bare[:, n_in:], 96)
        codes = []
        got = pg.prove_witness_batch_dev(r1cs, params, dw, rs, ss, check=True, solver=solver, finish=finish, _codes=codes)
        assert codes == [0, 0, 0] and [p.write() for p in got] == [p.write() for p in want], finish
        dw.release()
    public = cref.arr_to_ints(cref.fr_from_mont(np.ascontiguousarray(full[0, 1:n_in])))
    bellman_amd.verify_proof(bellman_amd.verifier.prepare_verifying_key(params), got[0], public)
    params.release()
    solver.release()
    r1cs.release()


def test_cpp_mirror(tmp_path):
    """the C++ mirror: Solver::solve_dev, prove_witness_batch_dev with both finishes and assemble_proofs against
    prove_witness (tests/cpp/prove_batch_dev_cubic.cpp)"""
    libdir = os.path.join(ROOT, "bellman_amd", "lib")
    exe = str(tmp_path / "prove_batch_dev_cubic.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "prove_batch_dev_cubic.cpp"), "-o", exe,
                           os.path.join(libdir, "libbellman_groth16.a"), "-L" + libdir, "-lbellman_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    gens = tmp_path / "gens.bin"
    gens.write_bytes(cref.g1_generator().tobytes() + cref.g2_generator().tobytes())
    r = subprocess.run([exe, str(gens)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "prove_batch_dev ok", (r.returncode, r.stdout, r.stderr)
