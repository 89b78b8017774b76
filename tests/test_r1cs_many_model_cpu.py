"""The integer model the GPU tests of the k-witness constraint evaluation and check are held against
(tests/models/r1cs_many_model.py), checked on its own: generated systems are satisfied by their solved witnesses, the first
unsatisfied constraint agrees with a brute-force walk, a corrupted wire is located where the model computes it, and the
Python captures of the MiMC and chain circuits are satisfied by their WitnessAssignment witnesses.  No GPU."""
import random

import pytest

from tests import circuits
from tests.models import r1cs_many_model as model

Q = model.Q
L = model.LONG_ROW
# row lengths (A, B) on both sides of the lane-per-row limit, at the limit, empty and single
LENGTHS = {0: (0, 1), 1: (1, 0), 2: (1, 1), 9: (L, 2), 10: (L + 1, 1), 11: (3, L + 1), 20: (3 * L + 5, 1), 21: (0, 0)}


@pytest.fixture(scope="module")
def system():
    return model.satisfiable_system(3, 6, 40, seed=11, lengths=LENGTHS)


def _witness(system, seed):
    rnd = random.Random(seed)
    inputs = [1] + [rnd.randrange(Q) for _ in range(system.n_in - 1)]
    free = [rnd.choice([0, 1, Q - 1, rnd.randrange(Q)]) for _ in range(system.n_aux - system.n_cons)]
    return inputs, model.solve(system, inputs, free)


def test_generator_shapes(system):
    assert system.n_cons == 40 and system.n_aux == 6 + 40
    assert {0, 1, Q - 1} <= set(system.table) and system.table[0] == 1
    assert {system.row_len(0, i) for i in range(40)} >= {0, 1, L, L + 1, 3 * L + 5}
    assert system.row_len(1, 11) == L + 1
    for i in range(40):   # the C row is one fresh aux variable with coefficient 1
        assert system.row(2, i) == [(3 + 6 + i, 1)]
        assert all(v < 3 + 6 + i for v, _ in system.row(0, i) + system.row(1, i))


def test_solved_witness_is_satisfied(system):
    for seed in range(3):
        inputs, aux = _witness(system, seed)
        assert len(aux) == system.n_aux
        assert model.first_bad(system, inputs, aux) is None and model.first_bad_brute(system, inputs, aux) is None
        a, b, c = model.evaluate(system, inputs, aux)
        assert all(x * y % Q == z for x, y, z in zip(a, b, c))


def test_corrupted_wire_is_located_by_the_model(system):
    rnd = random.Random(5)
    inputs, aux = _witness(system, 7)
    seen = set()
    for v in list(range(system.n_aux)):
        bad_aux = list(aux)
        bad_aux[v] = (bad_aux[v] + 1 + rnd.randrange(Q - 1)) % Q
        got = model.first_bad(system, inputs, bad_aux)
        assert got == model.first_bad_brute(system, inputs, bad_aux)
        if v >= system.n_aux - system.n_cons:   # the C variable of a constraint: that constraint can no longer hold
            assert got is not None
        seen.add(got)
    assert len(seen - {None}) > 10
    # two corrupted wires: the smaller index is reported
    bad_aux = list(aux)
    bad_aux[-1] = (bad_aux[-1] + 1) % Q
    bad_aux[-20] = (bad_aux[-20] + 1) % Q
    one = list(aux)
    one[-20] = bad_aux[-20]
    assert model.first_bad(system, inputs, bad_aux) == model.first_bad(system, inputs, one) == model.first_bad_brute(system, inputs, bad_aux)
    # input[0] = 0: whatever the model computes, both walks agree
    zero_in = [0] + inputs[1:]
    assert model.first_bad(system, zero_in, aux) == model.first_bad_brute(system, zero_in, aux)


def test_random_system_evaluates_like_a_plain_loop():
    s = model.random_system(2, 30, 50, seed=3, long_rows={(1, 7): L + 1})
    rnd = random.Random(1)
    inputs, aux = [1, rnd.randrange(Q)], [rnd.randrange(Q) for _ in range(30)]
    w = inputs + aux
    got = model.evaluate(s, inputs, aux)
    for mat in range(3):
        row_ptr, var, coeff = s.matrices[mat]
        assert got[mat] == [sum(s.table[coeff[t]] * w[var[t]] for t in range(row_ptr[i], row_ptr[i + 1])) % Q for i in range(50)]
    assert s.row_len(1, 7) == L + 1


def _captured(circuit_shape, circuit):
    from bellman_amd import groth16 as pg

    s = model.from_shape_assembly(pg.ShapeAssembly.capture(circuit_shape))
    w = pg.WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return s, w.input_assignment, w.aux_assignment


def test_python_captures_are_satisfied_by_their_witnesses():
    rnd = random.Random(322)
    cons = [rnd.randrange(Q) for _ in range(20)]
    xl, xr = rnd.randrange(Q), rnd.randrange(Q)
    s, inputs, aux = _captured(circuits.mimc_circuit(0, 0, cons), circuits.mimc_circuit(xl, xr, cons))
    assert (s.n_in, s.n_aux, s.n_cons) == (len(inputs), len(aux), 2 * 20 + s.n_in)
    assert model.first_bad(s, inputs, aux) is None
    bad = list(aux)
    bad[7] = (bad[7] + 1) % Q
    assert model.first_bad(s, inputs, bad) is not None and model.first_bad(s, inputs, bad) == model.first_bad_brute(s, inputs, bad)
    for rounds in (1, 61):
        s, inputs, aux = _captured(circuits.chain_circuit(rounds, 9, 0), circuits.chain_circuit(rounds, 9, 123456789))
        assert s.n_cons == rounds + 3 and model.first_bad(s, inputs, aux) is None
        bad = list(aux)
        bad[-1] = (bad[-1] + 5) % Q
        assert model.first_bad(s, inputs, bad) == model.first_bad_brute(s, inputs, bad) is not None


def test_cpp_checked_batch_example_builds():
    """tests/cpp/prove_batch_checked_cubic.cpp compiles and links against the in-tree libraries (it runs in
    tests/test_gpu_prove_batch_checked.py)"""
    import os

    from tests.test_gpu_prove_batch_checked import BIN, _build_cpp

    _build_cpp()
    assert os.path.exists(BIN)
