"""The batch prover behind a check of every witness (bh_groth16_prove_witness_batch_checked, prove_witness_batch(check=True)):
a witness with an unsatisfied constraint gets code 11, an all-zero slot and the constraint's index as the integer model
computes it (tests/models/r1cs_many_model.py); every other proof is prove_witness's, byte for byte.  And the grouped path
with the batched constraint evaluation (groth16.hpp BATCH_GROUPED_HE = 3, prove_witness_batch(_mode=3) through the test
library's bh_test_groth16_prove_witness_batch_he): every proof is prove_witness's, with one group and with several ragged ones."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cref
from oracle.cengine import CBls12
from oracle.pyref.generator import generate_parameters
from tests import circuits
from tests.models import r1cs_many_model as model
from tests.test_gpu_prove_batch_h import TOXIC, _chain_params, _domain, _equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "prove_batch_checked_cubic.bin")
Q = circuits.Q
UNSATISFIABLE = 11
SATISFIED = 0xFFFFFFFF
GROUPED_HE = 3


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def _witness(circuit):
    from bellman_amd import groth16 as pg

    w = pg.WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return w.input_assignment, w.aux_assignment


def _mimc_params(worker, cons):
    from bellman_amd import groth16 as pg

    p = generate_parameters(CBls12, circuits.mimc_circuit(0, 0, cons), CBls12.G1.gen, CBls12.G2.gen, **TOXIC)
    G1, G2 = CBls12.G1, CBls12.G2
    arr = lambda b: np.frombuffer(b, dtype=np.uint64)  # noqa: E731
    return pg.Parameters(worker, arr(p.vk.alpha_g1), arr(p.vk.beta_g1), arr(p.vk.beta_g2), arr(p.vk.delta_g1), arr(p.vk.delta_g2),
                         G1.to_array(p.h), G1.to_array(p.l), G1.to_array(p.a), G1.to_array(p.b_g1), G2.to_array(p.b_g2))


def _setup(worker, kind, k):
    """-> (r1cs, params, model system, k true witnesses) with the matrices captured from the Python circuit"""
    from bellman_amd import groth16 as pg

    rnd = random.Random(20)
    if kind == "mimc20":
        cons = [rnd.randrange(Q) for _ in range(20)]
        shape = circuits.mimc_circuit(0, 0, cons)
        pp = _mimc_params(worker, cons)
        wits = [_witness(circuits.mimc_circuit(rnd.randrange(Q), rnd.randrange(Q), cons)) for _ in range(k)]
    else:
        shape = circuits.chain_circuit(61, 68, 0)
        pp = _chain_params(worker, 61)
        wits = [_witness(circuits.chain_circuit(61, 68, 99 + j)) for j in range(k)]
    cs = pg.ShapeAssembly.capture(shape)
    matrices, table = cs.csr()
    r1cs = pg.R1CS.from_csr(worker, cs.num_inputs, cs.num_aux, matrices, table)
    return r1cs, pp, model.from_shape_assembly(cs), wits


def _corrupt(wit, position):
    aux = list(wit[1])
    aux[position] = (aux[position] + 1) % Q
    return list(wit[0]), aux


def _raw_checked(pp, r1cs, wits, rs, ss):
    """the C entry point itself, every output buffer pre-filled: -> (rc, proofs [k, 48], rcs, first_unsatisfied)"""
    from bellman_amd import _lib
    from bellman_amd.groth16 import fr_to_mont_array

    lib = _lib.load()
    k = len(wits)
    ins = np.ascontiguousarray(np.stack([fr_to_mont_array(list(w[0])) for w in wits]))
    auxs = np.ascontiguousarray(np.stack([fr_to_mont_array(list(w[1])) for w in wits]))
    rr, sv = fr_to_mont_array(list(rs)), fr_to_mont_array(list(ss))
    out = np.full((k, 48), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rcs = np.full(k, -77, dtype=np.int32)
    first = np.full(k, 12345, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.bh_groth16_prove_witness_batch_checked(pp._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k, p(rr), p(sv),
                                                    p(out), p(rcs), p(first), None)
    return rc, out, [int(c) for c in rcs], [None if int(b) == SATISFIED else int(b) for b in first]


@pytest.mark.parametrize("kind", ["mimc20", "chain61"])
def test_checked_batch_reports_unsatisfied_witnesses_and_proves_the_rest(worker, kind):
    import bellman_amd
    from bellman_amd import groth16 as pg

    k = 5
    r1cs, pp, system, wits = _setup(worker, kind, k)
    rnd = random.Random(5)
    wits[1] = _corrupt(wits[1], rnd.randrange(system.n_aux))
    wits[3] = _corrupt(wits[3], system.n_aux - 1)
    want_first = [model.first_bad(system, w_in, w_aux) for w_in, w_aux in wits]
    assert [w is None for w in want_first] == [True, False, True, False, True]
    rs, ss = [rnd.randrange(Q) for _ in range(k)], [rnd.randrange(Q) for _ in range(k)]
    singles = [pg.prove_witness(r1cs, pp, wits[j][0], wits[j][1], rs[j], ss[j]) for j in range(k)]
    rc, out, rcs, first = _raw_checked(pp, r1cs, wits, rs, ss)
    assert rc == 0 and rcs == [0, UNSATISFIABLE, 0, UNSATISFIABLE, 0] and first == want_first
    for j in range(k):
        if rcs[j]:
            assert not out[j].any()   # the slot of a refused witness is all zero
        else:
            assert _equal(pg.Proof(out[j].copy()), singles[j])
    # the Python call: per-proof codes on request, otherwise the first unsatisfied witness raises
    codes, reported = [], []
    proofs = pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], rs, ss, check=True, _codes=codes,
                                    _first_unsatisfied=reported)
    assert codes == rcs and reported == want_first
    assert [pr is None for pr in proofs] == [c != 0 for c in codes]
    assert all(_equal(proofs[j], singles[j]) for j in (0, 2, 4))
    with pytest.raises(bellman_amd.Unsatisfiable) as e:
        pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], rs, ss, check=True)
    assert e.value.index == want_first[1] and isinstance(e.value, bellman_amd.SynthesisError)
    # the unchecked call on the same batch still returns five proofs, as it always did
    unchecked = pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], rs, ss)
    assert len(unchecked) == k and all(_equal(unchecked[j], singles[j]) for j in range(k))
    # every witness bad; one witness, good and bad; none
    all_bad = [_corrupt(w, system.n_aux - 1 - j) for j, w in enumerate(wits)]
    rc, out, rcs, first = _raw_checked(pp, r1cs, all_bad, rs, ss)
    assert rc == 0 and rcs == [UNSATISFIABLE] * k and not out.any()
    assert first == [model.first_bad(system, w_in, w_aux) for w_in, w_aux in all_bad] and None not in first
    rc, out, rcs, first = _raw_checked(pp, r1cs, wits[:1], rs[:1], ss[:1])
    assert (rc, rcs, first) == (0, [0], [None]) and _equal(pg.Proof(out[0].copy()), singles[0])
    rc, out, rcs, first = _raw_checked(pp, r1cs, wits[1:2], rs[1:2], ss[1:2])
    assert (rc, rcs, first) == (0, [UNSATISFIABLE], want_first[1:2]) and not out.any()
    from bellman_amd import _lib
    assert _lib.load().bh_groth16_prove_witness_batch_checked(pp._h, r1cs._h, None, r1cs.num_inputs, None, r1cs.num_aux, 0, None, None,
                                                              None, None, None, None) == 0
    reported = [1]
    assert pg.prove_witness_batch(r1cs, pp, [], [], [], [], check=True, _first_unsatisfied=reported) == [] and reported == []
    with pytest.raises(AssertionError):   # a witness of the wrong shape refuses the whole call
        pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits[:-1]] + [wits[-1][1][:-1]], rs, ss, check=True)
    r1cs.release()


def _mode3_matches_singles(pg, r1cs, pp, ins, auxs, rs, ss):
    """k in {1, 3, 17} of the 17 witnesses: one group, and budgets that cut 3 into 2 + 1 and 17 into 5 + 5 + 5 + 2"""
    singles = [pg.prove_witness(r1cs, pp, ins[j], auxs[j], rs[j], ss[j]) for j in range(17)]
    vec = 4 * _domain(r1cs.num_constraints) * 32   # a, b, c and a scratch vector of one witness
    for k, budget in ((1, 0), (3, 0), (3, 2 * vec), (17, 0), (17, 5 * vec)):
        got = pg.prove_witness_batch(r1cs, pp, ins[:k], auxs[:k], rs[:k], ss[:k], _workspace_budget=budget, _mode=GROUPED_HE)
        assert len(got) == k
        for j in range(k):
            assert _equal(got[j], singles[j]), (k, budget, j)
    assert pg.prove_witness_batch(r1cs, pp, [], [], [], [], _mode=GROUPED_HE) == []


@pytest.mark.parametrize("rounds", [61, 4093])
def test_mode3_chain(worker, rounds):
    from bellman_amd import groth16 as pg

    seed = 7 + rounds
    pp = _chain_params(worker, rounds)
    r1cs = pg.R1CS.from_demo(worker, 1, rounds, seed)
    fs = [circuits.chain_assignment_fast(rounds, seed, 123456789 + 1000 * j) for j in range(17)]
    _mode3_matches_singles(pg, r1cs, pp, [f["input_assignment"] for f in fs], [f["aux_assignment"] for f in fs],
                           [0x1234567 + rounds + j for j in range(17)], [0x7654321 + 3 * j for j in range(17)])
    r1cs.release()


def test_mode3_mimc_322(worker):
    from bellman_amd import groth16 as pg

    rnd = random.Random(322)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    pp = _mimc_params(worker, cons)
    r1cs = pg.R1CS.from_circuit(worker, circuits.mimc_circuit(0, 0, cons))
    wits = [_witness(circuits.mimc_circuit(rnd.randrange(Q), rnd.randrange(Q), cons)) for _ in range(17)]
    _mode3_matches_singles(pg, r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], [rnd.randrange(Q) for _ in range(17)],
                           [rnd.randrange(Q) for _ in range(17)])
    r1cs.release()


def _build_cpp():
    from bellman_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = os.path.join(ROOT, "bellman_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "prove_batch_checked_cubic.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", BIN, os.path.join(lib, "libbellman_groth16.a"), "-L" + lib,
                           "-lbellman_hip", "-Wl,-rpath," + lib, "-lpthread"])


def test_cpp_checked_batch_matches_prove_witness(tmp_path):
    """the C++ mirror: R1cs::which_is_unsatisfied, prove_witness_batch_checked and BATCH_GROUPED_HE over witnesses that are
    not adjacent in host memory (tests/cpp/prove_batch_checked_cubic.cpp)"""
    _build_cpp()
    f = tmp_path / "gens.bin"
    f.write_bytes(cref.g1_generator().tobytes() + cref.g2_generator().tobytes())
    r = subprocess.run([BIN, str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == "prove_witness_batch_checked ok"
