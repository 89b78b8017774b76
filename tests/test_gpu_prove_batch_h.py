"""The grouped batch prover with a BATCHED h block (groth16.hpp BATCH_GROUPED_H, through the test library's
bh_test_groth16_prove_witness_batch_mode): a, b and c strided per witness, one bh_h_poly_fr_many_dev_on per group, then
the H many-job.  Every proof is prove_witness's and the grouped path's (mode 1), byte for byte, on MiMC-322 and on the
chain circuit at one constraint, 64 and 4096; a budget that cuts k = 5 into groups of 2, 2, 1 changes nothing; a witness of
the wrong shape refuses the whole call; the per-proof codes are those of mode 1."""
import random

import numpy as np
import pytest

from oracle import cref
from oracle.cengine import CBls12
from oracle.pyref.generator import generate_parameters
from tests import circuits

pytestmark = pytest.mark.gpu

TOXIC = dict(alpha=48577, beta=22580, gamma=53332, delta=5481, tau=3673)
Q = circuits.Q
GROUPED, GROUPED_H = 1, 2


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def _equal(p, q):
    return np.array_equal(p.a, q.a) and np.array_equal(p.b, q.b) and np.array_equal(p.c, q.c)


def _domain(n_constraints):
    m = 1
    while m < n_constraints:
        m *= 2
    return m


def _chain_params(worker, rounds, identity_in_h=False):
    """synthetic CRS for the chain circuit (distinct prime-order points; parity only)"""
    from bellman_amd import groth16 as pg

    m = _domain(rounds + 3)
    n_aux = rounds + 1
    nb = (rounds + 1) // 2 + 2
    h, l, a = cref.gen_bases(1, m - 1, a=11, b=3), cref.gen_bases(1, n_aux, a=5, b=7), cref.gen_bases(1, n_aux + 2, a=2, b=9)
    if identity_in_h:
        h[0] = 0   # the identity under a non-zero exponent: UnexpectedIdentity from the H multiexp of every proof
    b1, b2 = cref.gen_bases(1, nb, a=13, b=4), cref.gen_bases(2, nb, a=17, b=6)
    g1, g2 = cref.g1_generator(), cref.g2_generator()
    return pg.Parameters(worker, cref.point_mul(1, g1, 101), cref.point_mul(1, g1, 102), cref.point_mul(2, g2, 102),
                         cref.point_mul(1, g1, 103), cref.point_mul(2, g2, 103), h, l, a, b1, b2)


def _check_modes(pg, r1cs, pp, ins, auxs, rs, ss, budgets=(0,)):
    k = len(ins)
    singles = [pg.prove_witness(r1cs, pp, ins[j], auxs[j], rs[j], ss[j]) for j in range(k)]
    grouped = pg.prove_witness_batch(r1cs, pp, ins, auxs, rs, ss, _mode=GROUPED)
    for budget in budgets:
        got = pg.prove_witness_batch(r1cs, pp, ins, auxs, rs, ss, _workspace_budget=budget, _mode=GROUPED_H)
        assert len(got) == k
        for j in range(k):
            assert _equal(got[j], singles[j]) and _equal(got[j], grouped[j]), (budget, j)
    return singles


def test_mimc_322_batched_h_block(worker):
    from bellman_amd import groth16 as pg

    rnd = random.Random(322)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    p = generate_parameters(CBls12, circuits.mimc_circuit(0, 0, cons), CBls12.G1.gen, CBls12.G2.gen, **TOXIC)
    G1, G2 = CBls12.G1, CBls12.G2
    arr = lambda b: np.frombuffer(b, dtype=np.uint64)  # noqa: E731
    pp = pg.Parameters(worker, arr(p.vk.alpha_g1), arr(p.vk.beta_g1), arr(p.vk.beta_g2), arr(p.vk.delta_g1), arr(p.vk.delta_g2),
                       G1.to_array(p.h), G1.to_array(p.l), G1.to_array(p.a), G1.to_array(p.b_g1), G2.to_array(p.b_g2))
    r1cs = pg.R1CS.from_circuit(worker, circuits.mimc_circuit(0, 0, cons))
    k = 5
    cases = [tuple(rnd.randrange(Q) for _ in range(4)) for _ in range(k)]   # xl, xr, r, s
    ins, auxs = [], []
    for xl, xr, _, _ in cases:
        w = pg.WitnessAssignment()
        w.alloc_input(lambda: 1)
        circuits.mimc_circuit(xl, xr, cons)(w)
        ins.append(w.input_assignment)
        auxs.append(w.aux_assignment)
    m = _domain(r1cs.num_constraints)
    # the default budget (one group), and one that holds a, b, c and a scratch vector of two witnesses: groups of 2, 2, 1
    _check_modes(pg, r1cs, pp, ins, auxs, [c[2] for c in cases], [c[3] for c in cases], budgets=(0, 4 * 2 * m * 32))
    assert pg.prove_witness_batch(r1cs, pp, [], [], [], [], _mode=GROUPED_H) == []
    r1cs.release()


@pytest.mark.parametrize("rounds", [1, 61, 4093])
def test_chain_batched_h_block(worker, rounds):
    from bellman_amd import groth16 as pg

    seed, k = 7 + rounds, 5
    pp = _chain_params(worker, rounds)
    r1cs = pg.R1CS.from_demo(worker, 1, rounds, seed)
    fs = [circuits.chain_assignment_fast(rounds, seed, 123456789 + 1000 * j) for j in range(k)]
    rs = [0x1234567 + rounds + j for j in range(k)]
    ss = [0x7654321 + 3 * j for j in range(k)]
    m = _domain(rounds + 3)
    # groups of 5; of 2, 2, 1; of 1 (a budget below one witness still proves one at a time)
    _check_modes(pg, r1cs, pp, [f["input_assignment"] for f in fs], [f["aux_assignment"] for f in fs], rs, ss,
                 budgets=(0, 4 * 2 * m * 32, 1))
    r1cs.release()


def test_wrong_shape_refuses_the_whole_call(worker):
    from bellman_amd import groth16 as pg

    rounds, seed, k = 61, 68, 4
    pp = _chain_params(worker, rounds)
    r1cs = pg.R1CS.from_demo(worker, 1, rounds, seed)
    fs = [circuits.chain_assignment_fast(rounds, seed, 99 + j) for j in range(k)]
    ins = [f["input_assignment"] for f in fs]
    auxs = [list(f["aux_assignment"]) for f in fs]
    auxs[2] = auxs[2][:-1]
    with pytest.raises(AssertionError):
        pg.prove_witness_batch(r1cs, pp, ins, auxs, [1] * k, [2] * k, _mode=GROUPED_H)
    # ... and by the library itself: witness 2 of 4 one aux value short, in the call's own layout
    import ctypes

    from bellman_amd import _lib
    from bellman_amd.groth16 import fr_to_mont_array

    lib = _lib.load()
    ins_a = np.ascontiguousarray(np.stack([fr_to_mont_array(list(x)) for x in ins]))
    aux_a = np.ascontiguousarray(np.stack([fr_to_mont_array(list(f["aux_assignment"])) for f in fs]))
    rr, sv = fr_to_mont_array([1] * k), fr_to_mont_array([2] * k)
    out, rcs = np.zeros((k, 48), dtype=np.uint64), np.zeros(k, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for mode in (GROUPED, GROUPED_H):
        rc = lib.bh_test_groth16_prove_witness_batch_mode(pp._h, r1cs._h, p(ins_a), r1cs.num_inputs, p(aux_a), r1cs.num_aux - 1, k,
                                                          p(rr), p(sv), p(out), p(rcs), 0, mode, None)
        assert rc == -2 and not out.any(), mode
    assert lib.bh_test_groth16_prove_witness_batch_mode(pp._h, r1cs._h, p(ins_a), r1cs.num_inputs, p(aux_a), r1cs.num_aux, k,
                                                        p(rr), p(sv), p(out), p(rcs), 0, 3, None) == -2   # no such mode
    r1cs.release()


def test_per_proof_codes_are_those_of_the_grouped_path(worker):
    """an identity among the H bases under a non-zero exponent: UnexpectedIdentity per proof, from both modes alike; with
    the CRS intact both report success per proof"""
    from bellman_amd import groth16 as pg

    rounds, seed, k = 61, 68, 3
    r1cs = pg.R1CS.from_demo(worker, 1, rounds, seed)
    fs = [circuits.chain_assignment_fast(rounds, seed, 99 + j) for j in range(k)]
    ins, auxs = [f["input_assignment"] for f in fs], [f["aux_assignment"] for f in fs]
    for broken in (False, True):
        pp = _chain_params(worker, rounds, identity_in_h=broken)
        codes = {}
        for mode in (GROUPED, GROUPED_H):
            codes[mode] = []
            proofs = pg.prove_witness_batch(r1cs, pp, ins, auxs, [5, 6, 7], [8, 9, 10], _mode=mode, _codes=codes[mode])
            assert [pr is not None for pr in proofs] == [c == 0 for c in codes[mode]]
        assert codes[GROUPED_H] == codes[GROUPED]
        assert codes[GROUPED_H] == ([1] * k if broken else [0] * k)   # BH_ERR_UNEXPECTED_IDENTITY
    r1cs.release()
