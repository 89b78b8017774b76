"""The witness solver's planner (csrc/solve_plan.hpp through bh_test_r1cs_solve_plan, host only) against the integer
restatement of its rule (tests/models/r1cs_solve_model.py): which constraint or hint defines every variable, and at which
dependency level - on the three demo circuits with what they take from their `witness` argument supplied, on a few hundred
random circuits of synthesis-shaped gates, and on every refusal with the variable it reports.  The model's evaluation is held
against the circuits' own witnesses.  No GPU."""
import ctypes

import numpy as np
import pytest

from bellman_amd import _lib
from bellman_amd import groth16 as g
from tests import circuits
from tests.models import r1cs_solve_model as model

Q = model.Q


@pytest.fixture(scope="module")
def lib():
    if not _lib.os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def lib_plan(lib, n_inputs, n_aux, rows, supplied, hints):
    """-> (status, first_unsolved, definer list, level list, counts) of the C++ planner"""
    mats, table = model.csr(rows)
    keep = [tuple(np.asarray(x, dtype=np.uint32) for x in m) for m in mats]
    abc = (g._Csr * 3)(*[g._Csr(*[x.ctypes.data for x in m]) for m in keep])
    coeffs = g.fr_to_mont_array(table)
    desc, keep_desc = g.solver_desc(supplied, hints)
    n = n_inputs + n_aux
    bad = ctypes.c_uint32(12345)
    definer, level, counts = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint32), (ctypes.c_size_t * 5)()
    rc = lib.bh_test_r1cs_solve_plan(n_inputs, n_aux, len(rows[0]), ctypes.byref(abc), coeffs.ctypes.data, len(table), ctypes.byref(desc),
                                     ctypes.byref(bad), definer.ctypes.data, level.ctypes.data, counts)
    return rc, bad.value, [int(x) for x in definer], [int(x) for x in level], [int(x) for x in counts]


def assert_same_plan(lib, n_inputs, n_aux, rows, supplied, hints):
    p = model.plan(n_inputs + n_aux, rows, supplied, hints)
    rc, bad, definer, level, counts = lib_plan(lib, n_inputs, n_aux, rows, supplied, hints)
    assert (rc, bad) == (p.status, p.first_unsolved)
    if p.status == model.OK:
        assert definer == p.definer and level == p.level and counts == p.counts
    return p


def captured(circuit):
    cs = g.ShapeAssembly.capture(circuit)
    rows = tuple([[(idx if kind == g.INPUT else cs.num_inputs + idx, k) for kind, idx, k in row] for row in cs.rows[m]] for m in range(3))
    w = g.WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return cs.num_inputs, cs.num_aux, rows, w.input_assignment + w.aux_assignment


DEMOS = {
    "mimc": (lambda: circuits.mimc_circuit(3, 5, [(7 * i + 1) % Q for i in range(circuits.MIMC_ROUNDS)]), [0, 1]),
    "chain": (lambda: circuits.chain_circuit(65, 9, 12345), [0]),
    "boolmix": (lambda: circuits.boolmix_circuit(200, 4, 0xDEADBEEF12345), list(range(64))),
}


@pytest.mark.parametrize("name", sorted(DEMOS))
def test_demo_circuits_are_solved_from_what_they_take_from_outside(lib, name):
    """everything but the supplied aux variables comes out defined, the public outputs included; the model's values are the
    circuit's own"""
    make, supplied_aux = DEMOS[name]
    n_in, n_aux, rows, witness = captured(make())
    supplied = [n_in + a for a in supplied_aux]
    p = assert_same_plan(lib, n_in, n_aux, rows, supplied, [])
    assert p.status == model.OK and p.counts[:3] == [len(supplied), n_in + n_aux - 1 - len(supplied), 0]
    assert all(p.definer[v] >= 0 for v in range(1, n_in))
    start = [witness[v] if v == 0 or v in supplied else 0xBAD for v in range(n_in + n_aux)]
    assert model.complete(rows, [], p, start) == witness


@pytest.mark.parametrize("block", range(6))
def test_random_circuits(lib, block):
    for seed in range(50 * block, 50 * block + 50):
        c = model.random_circuit(seed, gates=12 + seed % 30)
        assert model.first_bad(c.rows, c.witness) is None
        p = assert_same_plan(lib, c.n_inputs, c.n_aux, c.rows, c.supplied, c.hints)
        assert p.status == model.OK, (seed, p.first_unsolved)
        start = [c.witness[v] if v == 0 or v in c.supplied else 0xBAD for v in range(c.n_vars)]
        assert model.complete(c.rows, c.hints, p, start) == c.witness, seed


def test_random_circuits_cover_every_gate():
    seen = set()
    general_s = zero_terms = 0
    for seed in range(60):
        c = model.random_circuit(seed)
        seen |= {k for k, _, _, _ in c.hints}
        zero_terms += sum(1 for m in range(3) for r in c.rows[m] for _, k in r if k == 0)
        p = model.plan(c.n_vars, c.rows, c.supplied, c.hints)
        for v, i in enumerate(p.definer):
            if i >= 0 and sum(k for x, k in c.rows[2][i] if x == v) % Q not in (1, Q - 1):
                general_s += 1
    assert seen == {model.BITS, model.INV_OR_ZERO} and general_s > 20 and zero_terms > 20


# variables: 0 ONE, 1 x, 2 y, 3 z;  x * x = y,  y * x = z
BASE = ([[(1, 1)], [(2, 1)]], [[(1, 1)], [(1, 1)]], [[(2, 1)], [(3, 1)]])


def _with(m, i, row):
    rows = tuple([list(r) for r in mat] for mat in BASE)
    rows[m][i] = row
    return rows


REFUSALS = {
    "a supplied variable withheld": (BASE, [], [], 1),
    "the variable also in A": (_with(0, 0, [(1, 1), (2, 5)]), [1], [], 2),
    "the variable in A with a zero coefficient is no obstacle": (_with(0, 0, [(1, 1), (2, 0)]), [1], [], None),
    "net coefficient zero": (_with(2, 0, [(2, 7), (2, Q - 7)]), [1], [], 2),
    "two unknowns in C": (_with(2, 0, [(2, 1), (3, 1)]), [1], [], 2),
    "a later constraint does not reach back": (([[(2, 1)], [(1, 1)]], [[(1, 1)], [(1, 1)]], [[(3, 1)], [(2, 1)]]), [1], [], 3),
    "a hint cycle": (_with(2, 0, []), [1], [(model.INV_OR_ZERO, [(3, 1)], [2], 0)], 2),
    "a hint writing ONE": (BASE, [1], [(model.BITS, [(1, 1)], [0], 0)], 0),
    "a hint writing a supplied variable": (BASE, [1], [(model.BITS, [(1, 1)], [1], 0)], 1),
    "two hints writing one variable": (_with(2, 0, []), [1], [(model.BITS, [(1, 1)], [2], 0), (model.INV_OR_ZERO, [(1, 1)], [2], 0)], 2),
    "bits beyond 256": (_with(2, 0, []), [1], [(model.BITS, [(1, 1)], [2], 256)], model.NO_VARIABLE),
    "the base circuit itself": (BASE, [1], [], None),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_report_the_variable(lib, name):
    rows, supplied, hints, reported = REFUSALS[name]
    p = assert_same_plan(lib, 1, 3, rows, supplied, hints)
    if reported is None:
        assert p.status == model.OK
    else:
        assert (p.status, p.first_unsolved) == (model.INVALID, reported)


def test_levels_of_the_base_circuit(lib):
    p = assert_same_plan(lib, 1, 3, BASE, [1], [])
    assert p.definer == [-1, -1, 0, 1] and p.level == [0, 0, 1, 2] and p.counts == [1, 2, 0, 2, 1]
    # a hint may read what a later constraint defines: y = 1 / x (hint), z = y * x, w = bits of z
    rows = ([[(2, 1)]], [[(1, 1)]], [[(3, 1)]])
    hints = [(model.BITS, [(3, 1)], [4, 5], 3), (model.INV_OR_ZERO, [(1, 1)], [2], 0)]
    p = assert_same_plan(lib, 1, 5, rows, [1], hints)
    assert p.definer == [-1, -1, -3, 0, -2, -2] and p.level == [0, 0, 1, 2, 3, 3]


def test_planner_under_host_sanitizers(tmp_path):
    """csrc/solve_plan.hpp in a stand-alone program of its own (tests/cpp/solve_plan_san.cpp, a toy field), built with
    AddressSanitizer and UndefinedBehaviorSanitizer and run as a process: nothing loaded into Python is involved"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "solve_plan_san.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "cpp", "solve_plan_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "solve_plan ok", (r.returncode, r.stdout, r.stderr)
