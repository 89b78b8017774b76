"""Parameters from a powers-of-tau transcript, CPU side: the plain model (tests/ptau_model.py) against the oracle's
generate_parameters with gamma = delta = 1 - the transcript is made from known (tau, alpha, beta), so the two must give
the same group elements - and the three entry points in the header, the ctypes table and the export map."""

import os
import random
import re

import pytest

from oracle.cengine import CBls12
from oracle.pyref import bls12_381 as bls
from oracle.pyref import errors as oerr
from oracle.pyref.generator import generate_parameters
from tests import circuits, ptau_model

Q = bls.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("bh_groth16_generate_from_powers_of_tau", "bh_groth16_params_rescale_delta", "bh_r1cs_eval_transposed_points_dev")

_rnd = random.Random(2718)
# (name, circuit, domain size).  boolmix_circuit opens with 64 bit checks, so its smallest domain is 128, not 64.
CASES = [
    ("mimc", circuits.mimc_circuit(0, 0, [_rnd.randrange(Q) for _ in range(5)]), 16),
    ("chain", circuits.chain_circuit(9, 20, 0), 16),
    ("chain-full-domain", circuits.chain_circuit(13, 3, 0), 16),
    ("forms", circuits.forms_circuit(10, 5, 77), 16),
    ("random", circuits.random_circuit(12, 9, 1234), None),
    ("boolmix", circuits.boolmix_circuit(0, 4, 99), 128),
]


def _oracle(circuit, toxic, delta=1):
    return generate_parameters(CBls12, circuit, CBls12.G1.gen, CBls12.G2.gen, alpha=toxic["alpha"], beta=toxic["beta"], gamma=1,
                               delta=delta, tau=toxic["tau"])


@pytest.mark.parametrize("name,circuit,want_m", CASES, ids=[c[0] for c in CASES])
def test_model_equals_the_known_tau_generator(name, circuit, want_m):
    rnd = random.Random(sum(map(ord, name)))
    toxic = dict(alpha=rnd.randrange(1, Q), beta=rnd.randrange(1, Q), tau=rnd.randrange(2, Q))
    m = ptau_model.domain_size(ptau_model.assemble(circuit).num_constraints)
    assert m <= 128 and (want_m is None or m == want_m)
    # a transcript longer than needed in every vector: only the prefixes count
    tr = ptau_model.transcript(toxic["tau"], toxic["alpha"], toxic["beta"], 2 * m + 2, m + 3)
    got = ptau_model.derive(circuit, tr)
    assert ptau_model.same_parameters(got, _oracle(circuit, toxic)) is None
    # the delta rescale, once and as two contributions
    d1, d2 = rnd.randrange(2, Q), rnd.randrange(2, Q)
    assert ptau_model.same_parameters(ptau_model.rescale_delta(got, d1), _oracle(circuit, toxic, delta=d1)) is None
    twice = ptau_model.rescale_delta(ptau_model.rescale_delta(got, d1), d2)
    assert ptau_model.same_parameters(twice, _oracle(circuit, toxic, delta=d1 * d2 % Q)) is None


def test_model_errors():
    circuit = circuits.chain_circuit(9, 20, 0)
    m = ptau_model.domain_size(ptau_model.assemble(circuit).num_constraints)
    for short in range(4):   # one point short in any of the four vectors
        tr = ptau_model.transcript(5, 6, 7, 2 * m - 1, m)
        vec = (tr.tau_g1, tr.tau_g2, tr.alpha_tau_g1, tr.beta_tau_g1)[short]
        vec.pop()
        with pytest.raises(oerr.PolynomialDegreeTooLarge):
            ptau_model.derive(circuit, tr)
    # alpha = -beta cancels (at*beta + bt*alpha + ct) for a variable used identically in A and B (generator.rs:464-470)
    shape = circuits.chain_circuit(2, 13, 0)
    with pytest.raises(oerr.UnconstrainedVariable):
        _oracle(shape, dict(alpha=5, beta=Q - 5, tau=987654323))
    with pytest.raises(oerr.UnconstrainedVariable):
        m2 = ptau_model.domain_size(ptau_model.assemble(shape).num_constraints)
        ptau_model.derive(shape, ptau_model.transcript(987654323, 5, Q - 5, 2 * m2 - 1, m2))
    with pytest.raises(oerr.UnexpectedIdentity):
        ptau_model.rescale_delta(ptau_model.derive(circuit, ptau_model.transcript(5, 6, 7, 2 * m - 1, m)), 0)


def test_entry_points_declared_bound_and_exported():
    """what this feature adds to the boundary; that EVERY declared entry point is bound, exported, in ffi.rs and in the
    version script is tests/test_abi_cpu.py::test_every_entry_point_is_declared_bound_and_exported"""
    header = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
    assert "bh_powers_of_tau;" in header
    assert re.search(r"VALIDATES NOTHING", header)   # the transcript call must say that it checks no point
    ffi = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")).read()
    assert "pub struct BhPowersOfTau" in ffi
