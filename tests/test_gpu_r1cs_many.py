"""k witnesses against one circuit in one GPU call: bh_r1cs_eval_many_dev (a = A.w, b = B.w, c = C.w of every witness) and
bh_r1cs_check_many_dev / bh_r1cs_check_many (the first constraint with a * b != c per witness - the reference's
TestConstraintSystem::which_is_unsatisfied).  Expected values come from the integer model (tests/models/r1cs_many_model.py)
only; the evaluation is also byte-identical to bh_r1cs_eval_dev per witness.  k sits on the edges of the kernels' witness
tile, strides are tight and loose, and every gap and a guard behind each buffer must come back as they were filled."""
import ctypes
import random

import numpy as np
import pytest

from tests import circuits
from tests.models import r1cs_many_model as model

pytestmark = pytest.mark.gpu

Q = model.Q
L = model.LONG_ROW
SENTINEL = 0xA5
GUARD = 256
SATISFIED = 0xFFFFFFFF


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


@pytest.fixture(scope="module")
def tile_ks(lib):
    t = lib.bh_test_r1cs_many_tile()
    assert t in (2, 4, 8)
    return sorted({1, t - 1, t, t + 1, 2 * t + 1} - {0})


class Dev:
    """a device buffer that starts as a copy of `image` (uint8)"""

    def __init__(self, lib, ctx, image):
        self.lib, self.ctx, self.n = lib, ctx, image.nbytes
        self.p = ctypes.c_void_p()
        assert lib.bh_dev_alloc(ctx, self.n, ctypes.byref(self.p)) == 0
        assert lib.bh_dev_upload(ctx, self.p, image.ctypes.data_as(ctypes.c_void_p), self.n) == 0

    def read(self):
        out = np.zeros(self.n, dtype=np.uint8)
        assert self.lib.bh_dev_download(self.ctx, out.ctypes.data_as(ctypes.c_void_p), self.p, self.n) == 0
        return out

    def free(self):
        self.lib.bh_dev_free(self.ctx, self.p)


def _mont_bytes(values):
    from bellman_amd.groth16 import fr_to_mont_array

    return fr_to_mont_array(list(values)).view(np.uint8).reshape(-1)


def _strided(vectors, stride):
    """vector j at j * stride in a sentinel-filled image with a guard behind it"""
    image = np.full(len(vectors) * stride + GUARD, SENTINEL, dtype=np.uint8)
    for j, v in enumerate(vectors):
        image[j * stride:j * stride + v.size] = v
    return image


def _register(worker, system):
    from bellman_amd import groth16 as pg

    return pg.R1CS.from_csr(worker, system.n_in, system.n_aux, system.matrices, system.table)


def _log_m(n_cons):
    log_m = 0
    while (1 << log_m) < n_cons:
        log_m += 1
    return log_m


def _random_witness(system, rnd):
    return ([1] + [rnd.randrange(Q) for _ in range(system.n_in - 1)],
            [rnd.choice([0, 1, rnd.randrange(Q)]) for _ in range(system.n_aux)])


# ---- evaluation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_in,n_aux,n_cons,seed", [(1, 0, 1, 1), (1, 1, 1, 2), (3, 40, 64, 3), (2, 500, 1000, 4), (5, 3000, 4097, 5)])
def test_eval_many_matches_model_and_single_eval(worker, lib, tile_ks, n_in, n_aux, n_cons, seed):
    long_rows = None
    if n_cons > 4000:   # rows above the lane-per-row limit at two indices of every matrix: summed by a workgroup per tile
        long_rows = {(mat, i): n for mat in range(3) for i, n in ((7 + mat, L + 1), (4000 + mat, 3 * L + 1))}
    system = model.random_system(n_in, n_aux, n_cons, seed, long_rows)
    r1cs = _register(worker, system)
    rnd = random.Random(seed)
    k_max = tile_ks[-1]
    wits = [_random_witness(system, rnd) for _ in range(k_max)]
    if k_max > 1:
        wits[1][0][0] = 0   # a witness whose input[0] is not the constant 1
    log_min = _log_m(n_cons)
    want = []   # per witness: the a, b, c vectors as bytes, zero padded to the minimal domain
    for w_in, w_aux in wits:
        abc = model.evaluate(system, w_in, w_aux)
        single = r1cs.eval(w_in, w_aux)
        vecs = []
        for mat in range(3):
            v = np.zeros((1 << log_min) * 32, dtype=np.uint8)
            v[:n_cons * 32] = _mont_bytes(abc[mat])
            assert np.array_equal(single[mat].view(np.uint8).reshape(-1), v)   # bh_r1cs_eval_dev, byte for byte
            vecs.append(v)
        want.append(vecs)
    ins = [_mont_bytes(w[0]) for w in wits]
    auxs = [_mont_bytes(w[1]) for w in wits]
    ctx = worker.ctx
    for k in tile_ks:
        for loose in (False, True):
            log_m = log_min + (1 if loose else 0)
            m_bytes = 32 << log_m
            in_stride, aux_stride, out_stride = n_in * 32 + 96 * loose, n_aux * 32 + 64 * loose, m_bytes + 96 * loose
            d_in, d_aux = Dev(lib, ctx, _strided(ins[:k], in_stride)), Dev(lib, ctx, _strided(auxs[:k], aux_stride))
            outs = [Dev(lib, ctx, np.full(k * out_stride + GUARD, SENTINEL, dtype=np.uint8)) for _ in range(3)]
            rc = lib.bh_r1cs_eval_many_dev(ctx, r1cs._h, d_in.p, in_stride, d_aux.p, aux_stride, k, outs[0].p, outs[1].p, outs[2].p,
                                           out_stride, log_m, None)
            assert rc == 0 and lib.bh_ctx_synchronize(ctx) == 0
            assert np.array_equal(d_in.read(), _strided(ins[:k], in_stride)) and np.array_equal(d_aux.read(), _strided(auxs[:k], aux_stride))
            for mat in range(3):
                got = outs[mat].read()
                for j in range(k):
                    vec = got[j * out_stride:j * out_stride + m_bytes]
                    assert np.array_equal(vec[:want[j][mat].size], want[j][mat]), (k, loose, mat, j)
                    assert not vec[n_cons * 32:].any()                                          # the zero padding up to 2^log_m
                    assert (got[j * out_stride + m_bytes:(j + 1) * out_stride] == SENTINEL).all()   # the gap behind vector j
                assert (got[k * out_stride:] == SENTINEL).all()                                  # the guard
            for d in [d_in, d_aux] + outs:
                d.free()
    # the Python hook: [k, m, 4] arrays, row j = eval of witness j
    got = r1cs.eval_many([w[0] for w in wits], [w[1] for w in wits])
    for mat in range(3):
        assert got[mat].shape == (k_max, 1 << log_min, 4)
        for j in range(k_max):
            assert np.array_equal(got[mat][j].view(np.uint8).reshape(-1), want[j][mat])
    r1cs.release()


# ---- check --------------------------------------------------------------------------------------------------------------

def _check_dev(worker, lib, r1cs, wits, loose):
    """bh_r1cs_check_many_dev over strided device copies; the verdict words carry a guard"""
    ctx, k = worker.ctx, len(wits)
    in_stride, aux_stride = r1cs.num_inputs * 32 + 64 * loose, r1cs.num_aux * 32 + 32 * loose
    ins, auxs = [_mont_bytes(w[0]) for w in wits], [_mont_bytes(w[1]) for w in wits]
    d_in, d_aux = Dev(lib, ctx, _strided(ins, in_stride)), Dev(lib, ctx, _strided(auxs, aux_stride))
    d_bad = Dev(lib, ctx, np.full(4 * k + GUARD, SENTINEL, dtype=np.uint8))
    rc = lib.bh_r1cs_check_many_dev(ctx, r1cs._h, d_in.p, in_stride, d_aux.p, aux_stride, k, d_bad.p, None)
    assert rc == 0 and lib.bh_ctx_synchronize(ctx) == 0
    got = d_bad.read()
    assert (got[4 * k:] == SENTINEL).all()
    assert np.array_equal(d_in.read(), _strided(ins, in_stride)) and np.array_equal(d_aux.read(), _strided(auxs, aux_stride))
    for d in (d_in, d_aux, d_bad):
        d.free()
    return [None if int(b) == SATISFIED else int(b) for b in got[:4 * k].view(np.uint32)]


def _assert_verdicts(worker, lib, r1cs, system, wits):
    """host form, device form (tight and loose strides) and the model agree; returns the verdicts"""
    want = [model.first_bad(system, w_in, w_aux) for w_in, w_aux in wits]
    assert r1cs.which_is_unsatisfied([w[0] for w in wits], [w[1] for w in wits]) == want
    assert _check_dev(worker, lib, r1cs, wits, False) == want
    assert _check_dev(worker, lib, r1cs, wits, True) == want
    return want


def _solved(system, rnd, input0=1):
    inputs = [input0] + [rnd.randrange(Q) for _ in range(system.n_in - 1)]
    free = [rnd.choice([0, 1, Q - 1, rnd.randrange(Q)]) for _ in range(system.n_aux - system.n_cons)]
    return inputs, model.solve(system, inputs, free)


def _corrupt(wit, aux_positions, rnd):
    aux = list(wit[1])
    for v in aux_positions:
        aux[v] = (aux[v] + 1 + rnd.randrange(Q - 1)) % Q
    return list(wit[0]), aux


def test_check_many_all_satisfied_on_the_tile_edges(worker, lib, tile_ks):
    system = model.satisfiable_system(3, 6, 300, seed=21, lengths={5: (L + 1, 2), 40: (2, L + 7), 299: (3 * L, 1), 7: (L, 1), 8: (0, 0)})
    r1cs = _register(worker, system)
    rnd = random.Random(1)
    wits = [_solved(system, rnd) for _ in range(tile_ks[-1])]
    for k in tile_ks:
        assert _assert_verdicts(worker, lib, r1cs, system, wits[:k]) == [None] * k
    assert r1cs.is_satisfied(*wits[0])
    r1cs.release()


def test_check_many_locates_the_first_unsatisfied_constraint(worker, lib, tile_ks):
    rnd = random.Random(2)
    # a long part in A, in B, and the LAST constraint long: its C variable is used nowhere else, so only that row fails
    system = model.satisfiable_system(3, 6, 300, seed=22, lengths={5: (L + 1, 2), 40: (2, L + 7), 299: (3 * L, 1)})
    r1cs = _register(worker, system)
    c_var = lambda i: system.n_aux - system.n_cons + i   # noqa: E731  (aux position of constraint i's C variable)
    good = _solved(system, rnd)
    wits = [
        _corrupt(good, [c_var(0)], rnd),                  # constraint 0
        _corrupt(good, [c_var(299)], rnd),                # only a long row
        good,
        _corrupt(good, [c_var(120), c_var(33)], rnd),     # two rows: the smaller is reported
        _corrupt(good, [c_var(5)], rnd),                  # a long A part
        _corrupt(good, [c_var(40)], rnd),                 # a long B part
        _corrupt(_solved(system, rnd, input0=0), [c_var(298)], rnd),   # input[0] = 0, bad near the end
        _solved(system, rnd, input0=0),                   # input[0] = 0, whatever the model says
        _corrupt(good, [2], rnd),                         # a free variable: wherever it is first used
    ]
    want = _assert_verdicts(worker, lib, r1cs, system, wits)
    assert want[0] == 0 and want[1] == 299 and want[2] is None and want[3] == 33 and want[4] == 5 and want[5] == 40
    assert len({w for w in want if w is not None}) >= 6   # different witnesses of one call are bad at different rows
    for k in tile_ks:   # every k on the tile edges, the bad witnesses in every slot of a tile
        for shift in range(2):
            batch = (wits[shift:] + wits[:shift])[:k]
            _assert_verdicts(worker, lib, r1cs, system, batch)
    assert not r1cs.is_satisfied(*wits[0])
    r1cs.release()
    # no long rows, the last real constraint of a domain-filling system
    small = model.satisfiable_system(2, 5, 64, seed=23)
    r1cs = _register(worker, small)
    good = _solved(small, rnd)
    last = _corrupt(good, [small.n_aux - 1], rnd)
    assert _assert_verdicts(worker, lib, r1cs, small, [good, last, good]) == [None, 63, None]
    r1cs.release()


def test_check_many_every_row_bad_from_an_index_on(worker, lib, tile_ks):
    """n_cons = 4097: the bad rows span many workgroups and many atomics per verdict word"""
    rnd = random.Random(3)
    system = model.satisfiable_system(3, 10, 4097, seed=24, lengths={7: (L + 1, 1), 4000: (1, 3 * L + 1)})
    r1cs = _register(worker, system)
    c_var = lambda i: system.n_aux - system.n_cons + i   # noqa: E731
    good = _solved(system, rnd)
    wits = [_corrupt(good, [c_var(i) for i in range(i0, 4097)], rnd) for i0 in (1900, 0, 4096)] + [good]
    wits = (wits * 3)[:tile_ks[-1]]
    want = _assert_verdicts(worker, lib, r1cs, system, wits)
    assert want[:3] == [1900, 0, 4096][:len(want)]
    r1cs.release()


def _captured(worker, shape, circuit):
    from bellman_amd import groth16 as pg

    cs = pg.ShapeAssembly.capture(shape)
    matrices, table = cs.csr()
    r1cs = pg.R1CS.from_csr(worker, cs.num_inputs, cs.num_aux, matrices, table)
    w = pg.WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return r1cs, model.from_shape_assembly(cs), (w.input_assignment, w.aux_assignment)


def _true_and_corrupted(worker, lib, r1cs, system, wit, seed):
    rnd = random.Random(seed)
    wits = [wit] + [_corrupt(wit, [rnd.randrange(system.n_aux)], rnd) for _ in range(4)]
    want = _assert_verdicts(worker, lib, r1cs, system, wits)
    assert want[0] is None and any(w is not None for w in want[1:])
    r1cs.release()


@pytest.mark.parametrize("rounds", [1, 61, 4093])
def test_check_many_chain_circuit(worker, lib, rounds):
    r1cs, system, wit = _captured(worker, circuits.chain_circuit(rounds, 7 + rounds, 0), circuits.chain_circuit(rounds, 7 + rounds, 123456789))
    assert system.n_cons == rounds + 3
    _true_and_corrupted(worker, lib, r1cs, system, wit, rounds)


def test_check_many_mimc_322(worker, lib):
    rnd = random.Random(322)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    r1cs, system, wit = _captured(worker, circuits.mimc_circuit(0, 0, cons), circuits.mimc_circuit(rnd.randrange(Q), rnd.randrange(Q), cons))
    assert system.n_cons == 646
    _true_and_corrupted(worker, lib, r1cs, system, wit, 322)


def test_check_many_boolean_demo_circuit(worker, lib):
    rounds = circuits.boolmix_rounds(8)
    r1cs, system, wit = _captured(worker, circuits.boolmix_circuit(rounds, 5, 0), circuits.boolmix_circuit(rounds, 5, 0x1234567))
    _true_and_corrupted(worker, lib, r1cs, system, wit, 8)


# ---- argument errors ------------------------------------------------------------------------------------------------------

def test_argument_errors(worker, lib):
    system = model.satisfiable_system(2, 3, 9, seed=31)
    r1cs = _register(worker, system)
    ctx = worker.ctx
    n_in, n_aux = system.n_in, system.n_aux
    wit = _solved(system, random.Random(4))
    d_in, d_aux = Dev(lib, ctx, _strided([_mont_bytes(wit[0])], n_in * 32)), Dev(lib, ctx, _strided([_mont_bytes(wit[1])], n_aux * 32))
    out = [Dev(lib, ctx, np.full(16 * 32 + GUARD, SENTINEL, dtype=np.uint8)) for _ in range(3)]
    bad = Dev(lib, ctx, np.full(4 + GUARD, SENTINEL, dtype=np.uint8))

    def ev(in_stride=n_in * 32, aux_stride=n_aux * 32, k=1, out_stride=16 * 32, log_m=4, r=r1cs._h, c=ctx):
        return lib.bh_r1cs_eval_many_dev(c, r, d_in.p, in_stride, d_aux.p, aux_stride, k, out[0].p, out[1].p, out[2].p, out_stride, log_m, None)

    def ck(in_stride=n_in * 32, aux_stride=n_aux * 32, k=1, r=r1cs._h, c=ctx):
        return lib.bh_r1cs_check_many_dev(c, r, d_in.p, in_stride, d_aux.p, aux_stride, k, bad.p, None)

    assert ev(in_stride=n_in * 32 - 32) == -2 and ck(in_stride=n_in * 32 - 32) == -2      # a stride below the vector
    assert ev(aux_stride=n_aux * 32 - 32) == -2 and ck(aux_stride=n_aux * 32 - 32) == -2
    assert ev(in_stride=n_in * 32 + 8) == -2 and ck(aux_stride=n_aux * 32 + 16) == -2     # not a multiple of 32
    assert ev(out_stride=16 * 32 - 32) == -2 and ev(out_stride=16 * 32 + 4) == -2
    assert ev(log_m=3, out_stride=8 * 32) == -2                                           # 2^3 < 9 constraints
    assert ev(r=None) == -2 and ck(r=None) == -2 and ev(c=None) == -2 and ck(c=None) == -2
    assert lib.bh_ctx_synchronize(ctx) == 0
    for d in out + [bad]:   # nothing ran
        assert (d.read() == SENTINEL).all()
    assert ev(k=0) == 0 and ck(k=0) == 0 and lib.bh_ctx_synchronize(ctx) == 0             # k = 0: BH_OK, nothing launched
    for d in out + [bad]:
        assert (d.read() == SENTINEL).all()
    assert lib.bh_r1cs_check_many(ctx, r1cs._h, None, None, 0, None) == 0
    assert lib.bh_r1cs_check_many(None, r1cs._h, None, None, 1, None) == -2
    assert r1cs.which_is_unsatisfied([], []) == []
    with pytest.raises(AssertionError):   # a witness of the wrong shape
        r1cs.which_is_unsatisfied([wit[0]], [wit[1][:-1]])
    assert ev() == 0 and ck() == 0 and lib.bh_ctx_synchronize(ctx) == 0                   # the same handles do run
    assert bad.read()[:4].view(np.uint32)[0] == SATISFIED
    for d in [d_in, d_aux, bad] + out:
        d.free()
    r1cs.release()
