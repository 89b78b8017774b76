"""The witness solver on the GPU (bh_r1cs_solver_create, bh_r1cs_solve_many_dev / bh_r1cs_solve_many, R1CS.solver,
prove_witness_batch(solver=...)): k witnesses completed in place from the values of their supplied variables.  Every byte of
every buffer is compared: the demo circuits against the host synthesis (bh_test_demo_assignment), random circuits and the
hints against the integer model (tests/models/r1cs_solve_model.py).  Buffers start with garbage in every slot the solver has
to write, strides are looser than the vectors with a sentinel in the gaps and a guard behind, k sits on the edges of a
wavefront and of a workgroup's group of witnesses, and both launch forms run on the same inputs."""
import ctypes
import random

import numpy as np
import pytest

from tests.models import r1cs_solve_model as model

pytestmark = pytest.mark.gpu

Q = model.Q
SENTINEL = 0xA5
GUARD = 256
KS = (1, 2, 3, 64, 65, 130)
AUTO, WALK, LEVEL = 0, 1, 2
MIMC, CHAIN, BOOLMIX = 0, 1, 5


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


def _mont(values):
    from bellman_amd.groth16 import fr_to_mont_array

    return fr_to_mont_array(list(values))


def _images(full, n_inputs, supplied, stride_extra, seed):
    """full: [k, n_vars, 4] uint64 expected witnesses -> per vector kind (inputs, aux): (start image, expected image, stride):
    witness j at j * stride; the start image holds ONE and the supplied variables, garbage in every other slot, the sentinel in
    the gaps and in a guard behind the last witness"""
    k, n_vars = full.shape[0], full.shape[1]
    keep = np.zeros(n_vars, dtype=bool)
    keep[[0] + list(supplied)] = True
    garbage = np.random.RandomState(seed).randint(0, 256, size=(k, n_vars, 32)).astype(np.uint8)
    start = np.where(keep[None, :, None], full.view(np.uint8).reshape(k, n_vars, 32), garbage)
    out = []
    for lo, hi in ((0, n_inputs), (n_inputs, n_vars)):
        stride = (hi - lo) * 32 + stride_extra
        imgs = []
        for src in (start, full.view(np.uint8).reshape(k, n_vars, 32)):
            img = np.full(k * stride + GUARD, SENTINEL, dtype=np.uint8)
            for j in range(k):
                img[j * stride:j * stride + (hi - lo) * 32] = src[j, lo:hi].reshape(-1)
            imgs.append(img)
        out.append((imgs[0], imgs[1], stride))
    return out


class Dev:
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


def _solve_dev(lib, worker, solver, full, n_inputs, supplied, k, form=AUTO, group=0, stride_extra=96, seed=1):
    """runs bh_r1cs_solve_many_dev on the first k witnesses; asserts every byte; returns the two result images"""
    ctx = worker.ctx
    (in0, in_want, in_stride), (aux0, aux_want, aux_stride) = _images(full[:k], n_inputs, supplied, stride_extra, seed)
    assert lib.bh_test_r1cs_solver_tune(solver._h, form, group, 0) == 0
    d_in, d_aux = Dev(lib, ctx, in0), Dev(lib, ctx, aux0)
    try:
        assert lib.bh_r1cs_solve_many_dev(ctx, solver._h, d_in.p, in_stride, d_aux.p, aux_stride, k, None) == 0
        assert lib.bh_ctx_synchronize(ctx) == 0
        got_in, got_aux = d_in.read(), d_aux.read()
    finally:
        d_in.free()
        d_aux.free()
        lib.bh_test_r1cs_solver_tune(solver._h, AUTO, 0, 0)
    assert np.array_equal(got_in, in_want), "inputs, form %d group %d k %d" % (form, group, k)
    assert np.array_equal(got_aux, aux_want), "aux, form %d group %d k %d" % (form, group, k)
    return got_in, got_aux


def _demo(worker, kind, size, k, seed=3):
    """-> (r1cs, solver, [k, n_vars, 4] host-synthesised witnesses, supplied variable indices)"""
    from bellman_amd import groth16 as pg

    rnd = random.Random(1000 * kind + size)
    constants = [rnd.randrange(Q) for _ in range(size)] if kind == MIMC else None
    r1cs = pg.R1CS.from_demo(worker, kind, size, seed, constants)
    n_sup = {MIMC: 2, CHAIN: 1, BOOLMIX: 64}[kind]
    con = _mont(constants) if constants else None
    rows = []
    for _ in range(k):
        wit = [rnd.randrange(Q), rnd.randrange(Q)] if kind == MIMC else [rnd.randrange(Q)]
        asg = pg.demo_assignment(kind, size, seed, wit, con)
        rows.append(np.concatenate([asg["input_assignment"], asg["aux_assignment"]]))
    full = np.ascontiguousarray(np.stack(rows))
    assert full.shape[1] == r1cs.num_inputs + r1cs.num_aux
    solver = r1cs.solver([pg.Variable(pg.AUX, a) for a in range(n_sup)])
    return r1cs, solver, full, [r1cs.num_inputs + a for a in range(n_sup)]


DEMOS = [(CHAIN, 1), (CHAIN, 2), (CHAIN, 63), (CHAIN, 64), (CHAIN, 65), (CHAIN, 300), (MIMC, 322), (BOOLMIX, 64), (BOOLMIX, 200)]


@pytest.mark.parametrize("kind,size", DEMOS)
def test_demo_circuits_every_k_and_both_forms(worker, lib, kind, size):
    r1cs, solver, full, supplied = _demo(worker, kind, size, max(KS))
    n_in = r1cs.num_inputs
    info = solver.info
    assert info["supplied"] == len(supplied) and info["hinted"] == 0
    assert info["defined"] == full.shape[1] - 1 - len(supplied)      # everything else, the public outputs included
    for k in KS:
        _solve_dev(lib, worker, solver, full, n_in, supplied, k, seed=k)
    # both forms forced on the same inputs (the bytes are the expected ones, so identical), groups of 1, 3 and 64 witnesses:
    # k = 65 leaves a ragged last group at 3 and at 64, k = 130 a second full group and a third of two
    _solve_dev(lib, worker, solver, full, n_in, supplied, 65, form=LEVEL, seed=7)
    for group in (1, 3, 64):
        _solve_dev(lib, worker, solver, full, n_in, supplied, 65, form=WALK, group=group, seed=7)
    _solve_dev(lib, worker, solver, full, n_in, supplied, 130, form=WALK, group=64, stride_extra=0, seed=8)
    # ... and the check agrees that the solved witnesses satisfy the circuit
    assert r1cs.which_is_unsatisfied(np.ascontiguousarray(full[:5, :n_in]), np.ascontiguousarray(full[:5, n_in:])) == [None] * 5
    spare = Dev(lib, worker.ctx, np.zeros(64, dtype=np.uint8))   # k = 0: nothing is launched, nothing is read
    assert lib.bh_r1cs_solve_many_dev(worker.ctx, solver._h, spare.p, n_in * 32, spare.p, r1cs.num_aux * 32, 0, None) == 0
    assert lib.bh_r1cs_solve_many_dev(worker.ctx, solver._h, spare.p, n_in * 32 - 32, spare.p, r1cs.num_aux * 32, 1, None) == -2
    spare.free()
    solver.release()
    r1cs.release()


def _register(worker, n_inputs, n_aux, rows):
    from bellman_amd import groth16 as pg

    mats, table = model.csr(rows)
    return pg.R1CS.from_csr(worker, n_inputs, n_aux, mats, table)


def _raw_solver(lib, worker, r1cs, supplied, hints):
    """a Solver from plain indices (the Python front door takes Variables and LinearCombinations)"""
    from bellman_amd import groth16 as pg

    desc, keep = pg.solver_desc(supplied, hints)
    bad, h = ctypes.c_uint32(0), ctypes.c_void_p()
    assert lib.bh_r1cs_solver_create(worker.ctx, r1cs._h, ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(h)) == 0
    return pg.Solver(r1cs, h)


def _model_witnesses(rows, hints, supplied, n_vars, starts):
    p = model.plan(n_vars, rows, supplied, hints)
    assert p.status == model.OK
    wits = [model.complete(rows, hints, p, s) for s in starts]
    return p, np.ascontiguousarray(np.stack([_mont(w) for w in wits])), wits


@pytest.mark.parametrize("seed", range(10))
def test_random_circuits_match_the_model(worker, lib, seed):
    c = model.random_circuit(100 + seed, gates=30 + 3 * seed)
    rnd = random.Random(seed)
    starts = [list(c.witness)]
    for _ in range(4):   # other supplied values: bits stay bits, everything else is any field element
        starts.append([(rnd.randrange(2) if c.witness[v] in (0, 1) else rnd.choice([0, 1, Q - 1, rnd.randrange(Q)]))
                       if v in c.supplied else c.witness[v] for v in range(c.n_vars)])
    p, full, wits = _model_witnesses(c.rows, c.hints, c.supplied, c.n_vars, starts)
    assert wits[0] == c.witness
    assert all(model.first_bad(c.rows, w) is None for w in wits)
    r1cs = _register(worker, c.n_inputs, c.n_aux, c.rows)
    solver = _raw_solver(lib, worker, r1cs, c.supplied, c.hints)
    assert [solver.info[x] for x in ("supplied", "defined", "hinted", "levels", "widest_level")] == p.counts
    for k in (1, 5):
        _solve_dev(lib, worker, solver, full, c.n_inputs, c.supplied, k, seed=seed)
    _solve_dev(lib, worker, solver, full, c.n_inputs, c.supplied, 5, form=LEVEL, seed=seed)
    _solve_dev(lib, worker, solver, full, c.n_inputs, c.supplied, 5, form=WALK, group=2, seed=seed)
    n_in = c.n_inputs
    assert r1cs.which_is_unsatisfied(np.ascontiguousarray(full[:, :n_in]), np.ascontiguousarray(full[:, n_in:])) == [None] * 5
    solver.release()
    r1cs.release()


def test_hints_at_their_corner_values(worker, lib):
    """BITS at shift 0 and at a shift > 0, of values >= 2^64 and of q - 1; INV_OR_ZERO at 0 and at 1; a combination with
    coefficients of the hints' own table; a defined variable that reads hint outputs"""
    # variables: 0 ONE, 1 x, 2 y (supplied); 3..258 all 256 bits of x; 259..358 bits 70..169 of 3x + y; 359 1/y or 0;
    # 360 = x * (1/y) by a constraint;  361 1/(x - y) or 0
    rows = ([[(1, 1)]], [[(359, 1)]], [[(360, 1)]])
    hints = [(model.BITS, [(1, 1)], list(range(3, 259)), 0),
             (model.BITS, [(1, 3), (2, 1)], list(range(259, 359)), 70),
             (model.INV_OR_ZERO, [(2, 1)], [359], 0),
             (model.INV_OR_ZERO, [(1, 1), (2, Q - 1)], [361], 0)]
    n_vars = 362
    xs = [(Q - 1, 0), ((1 << 64) + 5, 1), ((1 << 200) + (1 << 64) - 1, Q - 1), (0, 0), (12345, 12345), (0x9E3779B97F4A7C15 << 130, 7)]
    starts = [[1, x, y] + [0] * (n_vars - 3) for x, y in xs]
    p, full, wits = _model_witnesses(rows, hints, [1, 2], n_vars, starts)
    assert wits[0][3:258] == [(Q - 1 >> j) & 1 for j in range(255)] and wits[0][359] == 0 and wits[1][359] == 1 and wits[4][361] == 0
    assert sum(wits[5][259:359]) > 8 and sum(wits[2][3:259]) == 65
    r1cs = _register(worker, 1, n_vars - 1, rows)
    solver = _raw_solver(lib, worker, r1cs, [1, 2], hints)
    assert p.counts == [2, 1, 358, 2, 4] and [solver.info[x] for x in ("supplied", "defined", "hinted", "levels", "widest_level")] == p.counts
    for form, group in ((AUTO, 0), (LEVEL, 0), (WALK, 4)):
        _solve_dev(lib, worker, solver, full, 1, [1, 2], len(xs), form=form, group=group)
    solver.release()
    r1cs.release()


def test_host_form_and_python_front_door(worker, lib):
    """bh_r1cs_solve_many (Solver.solve / solve_many) returns what the device form leaves in the buffers; the inputs are not
    touched; creation refuses an undetermined variable by name"""
    from bellman_amd import groth16 as pg

    r1cs, solver, full, supplied = _demo(worker, CHAIN, 65, 7)
    n_in = r1cs.num_inputs
    _solve_dev(lib, worker, solver, full, n_in, supplied, 7)
    start = full.copy()
    start[:, 1:n_in] = 0x1111
    start[:, n_in + 1:] = 0x2222
    before = start.copy()
    ins, auxs = solver.solve_many(np.ascontiguousarray(start[:, :n_in]), np.ascontiguousarray(start[:, n_in:]))
    assert np.array_equal(start, before)
    assert np.array_equal(ins, full[:, :n_in]) and np.array_equal(auxs, full[:, n_in:])
    x0 = int.from_bytes(bytes(full[2, n_in].view(np.uint8)), "little") * pow(1 << 256, -1, Q) % Q
    i1, a1 = solver.solve([1] + [0] * (n_in - 1), [x0] + [0] * (r1cs.num_aux - 1))
    assert np.array_equal(i1, full[2, :n_in]) and np.array_equal(a1, full[2, n_in:])
    assert solver.solve_many([], [])[0].shape[0] == 0
    with pytest.raises(ValueError, match=r"Variable\(INPUT, 1\)"):   # nothing supplied: the lowest unknown is the public output
        r1cs.solver([])
    with pytest.raises(ValueError, match=r"Variable\(INPUT, 0\)"):
        r1cs.solver([pg.Variable(pg.AUX, 0)], [pg.BitsHint(pg.LinearCombination() + pg.Variable(pg.AUX, 0), [pg.Variable(pg.INPUT, 0)])])
    solver.release()
    r1cs.release()


def _params(worker, r1cs):
    from bellman_amd import groth16 as pg
    from oracle.cengine import CBls12

    g1, g2 = (np.frombuffer(bytes(g), dtype=np.uint64) for g in (CBls12.G1.gen, CBls12.G2.gen))
    return pg.Parameters.generate(worker, r1cs, g1, g2, 48577, 22580, 53332, 5481, 3673)


def test_batch_prover_through_the_solver(worker):
    """prove_witness_batch(solver=...) on MiMC-322 x 3: the proofs of the host-synthesised witnesses with the same r, s,
    byte for byte, from buffers that hold nothing but ONE, xl and xr"""
    from bellman_amd import groth16 as pg

    r1cs, solver, full, supplied = _demo(worker, MIMC, 322, 3)
    n_in = r1cs.num_inputs
    params = _params(worker, r1cs)
    rs, ss = [11, 22, 33], [44, 55, 66]
    want = pg.prove_witness_batch(r1cs, params, np.ascontiguousarray(full[:, :n_in]), np.ascontiguousarray(full[:, n_in:]), rs, ss)
    bare = np.zeros_like(full)
    bare[:, [0] + supplied] = full[:, [0] + supplied]
    got = pg.prove_witness_batch(r1cs, params, np.ascontiguousarray(bare[:, :n_in]), np.ascontiguousarray(bare[:, n_in:]), rs, ss,
                                 solver=solver, check=True)
    assert [p.write() for p in got] == [p.write() for p in want]
    params.release()
    solver.release()
    r1cs.release()


def test_corrupted_supplied_value_is_solved_and_then_named_by_the_check(worker):
    """a state bit of the boolean circuit set to 2: every variable is still computed, and the check that follows names the
    witness (errors.Unsatisfiable / code 11) at the bit's own boolean constraint"""
    import bellman_amd
    from bellman_amd import groth16 as pg

    r1cs, solver, full, supplied = _demo(worker, BOOLMIX, 64, 3)
    n_in = r1cs.num_inputs
    params = _params(worker, r1cs)
    bare = np.zeros_like(full)
    bare[:, [0] + supplied] = full[:, [0] + supplied]
    bare[1, supplied[5]] = _mont([2])[0]
    ins, auxs = np.ascontiguousarray(bare[:, :n_in]), np.ascontiguousarray(bare[:, n_in:])
    solved_in, solved_aux = solver.solve_many(ins, auxs)
    assert np.array_equal(solved_in[[0, 2]], full[[0, 2], :n_in]) and np.array_equal(solved_aux[[0, 2]], full[[0, 2], n_in:])
    assert r1cs.which_is_unsatisfied(solved_in, solved_aux) == [None, 5, None]
    codes, first = [], []
    proofs = pg.prove_witness_batch(r1cs, params, ins, auxs, [1, 2, 3], [4, 5, 6], solver=solver, check=True, _codes=codes,
                                    _first_unsatisfied=first)
    assert codes == [0, 11, 0] and first == [None, 5, None] and proofs[1] is None and proofs[0] is not None
    with pytest.raises(bellman_amd.Unsatisfiable) as e:
        pg.prove_witness_batch(r1cs, params, ins, auxs, [1, 2, 3], [4, 5, 6], solver=solver, check=True)
    assert e.value.index == 5
    params.release()
    solver.release()
    r1cs.release()


def test_cpp_mirror_solver(tmp_path):
    """the C++ mirror: R1cs::solver / Solver::solve against the circuit's own synthesis (tests/cpp/solve_cubic.cpp)"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "bellman_amd", "lib")
    exe = str(tmp_path / "solve_cubic.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(root, "tests", "cpp", "solve_cubic.cpp"), "-o", exe,
                           os.path.join(libdir, "libbellman_groth16.a"), "-L" + libdir, "-lbellman_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "solver ok", (r.returncode, r.stdout, r.stderr)
