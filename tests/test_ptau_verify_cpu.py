"""The powers-of-tau check without a GPU: the host build of the coefficient expander (csrc/ptau_rlc.cuh through
bh_test_ptau_rlc_host) against hashlib, the exponent model (tests/models/ptau_verify_model.py) against real pairings of
oracle/pyref, and the new entry points in the header, the ctypes table, the export map, the library and the generated
Rust declarations."""

import ctypes
import os
import re

import numpy as np
import pytest

from oracle.pyref import bls12_381 as bls
from oracle.pyref import pairing
from tests.models import ptau_verify_model as model

Q = bls.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("bh_bases_validate", "bh_pairing_product_is_one", "bh_powers_of_tau_verify")
SEEDS = (bytes(range(32)), bytes(255 - 7 * i % 256 for i in range(32)))


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seed1"])
@pytest.mark.parametrize("v", [0, 1, 2, 3])
@pytest.mark.parametrize("count", [1, 2, 3, 129])
def test_host_expander_equals_hashlib(seed, v, count):
    from bellman_amd import _lib

    lib = _lib.load()
    out = np.full((count + 1) * 32, 0xA5, dtype=np.uint8)   # one scalar of guard: an odd count drops the last half block
    lib.bh_test_ptau_rlc_host(seed, v, count, out.ctypes.data_as(ctypes.c_void_p))
    assert out[:count * 32].tobytes() == model.coefficient_bytes(seed, v, count)
    assert (out[count * 32:] == 0xA5).all()


def test_coefficients_are_128_bit_and_differ_by_vector():
    rho = [model.coefficients(SEEDS[0], v, 5) for v in range(4)]
    assert all(0 <= r < 1 << 128 for v in rho for r in v)
    assert len({tuple(v) for v in rho}) == 4
    assert model.coefficients(SEEDS[0], 0, 5)[:4] == model.coefficients(SEEDS[0], 0, 4)


def _pairing_says(eq):
    _, a, b, c, d = eq
    g1 = lambda k: bls.G1.mul(bls.G1.gen, k) if k else None  # noqa: E731
    g2 = lambda k: bls.G2.mul(bls.G2.gen, k) if k else None  # noqa: E731
    return pairing.pairing_product_is_one([(g1(a), g2(b)), (bls.G1.neg(g1(c)) if c else None, g2(d))])


@pytest.mark.parametrize("which", ["consistent", "inconsistent"])
def test_exponent_model_equals_real_pairings(which):
    """the six equations of a transcript with vectors of three points, evaluated by oracle/pyref's Miller loop and final
    exponentiation, hold exactly where the model's products agree mod q"""
    tr = model.Transcript.consistent(tau=0x1234567, alpha=0x89ABC, beta=0xDEF01, n1=3, n=3)
    if which == "inconsistent":   # one fault in every equation
        tr.vec[0][2] += 1        # TAU_G1
        tr.vec[1][1] += 1        # TAU_G1_G2, TAU_G2 (and s2 enters TAU_G1, ALPHA, BETA)
        tr.vec[2][1] += 1        # ALPHA
        tr.vec[3][2] += 1        # BETA
        tr.beta2 += 1            # BETA_G2
        tr = tr.copy()
    eqs = model.equations(tr, SEEDS[0])
    assert [e[0] for e in eqs] == [model.TAU_G1_G2, model.TAU_G1, model.TAU_G2, model.ALPHA, model.BETA, model.BETA_G2]
    got = 0
    for eq in eqs:
        if not _pairing_says(eq):
            got |= eq[0]
    assert got == model.mask(tr, SEEDS[0])
    assert got == (0 if which == "consistent" else 0x7E)


def test_model_masks():
    seed = SEEDS[1]
    tr = model.Transcript.consistent(5, 6, 7, 9, 4)
    assert model.mask(tr, seed) == 0
    one = model.Transcript.consistent(5, 6, 7, 2, 2)
    one.vec[2], one.vec[3] = one.vec[2][:1], one.vec[3][:1]   # alpha and beta vectors of one point: vacuous
    assert model.mask(one, seed) == 0 and len(model.equations(one, seed)) == 4
    bad = tr.copy()
    bad.vec[0][0] = 0
    assert model.mask(bad, seed) == model.HEAD
    scaled = tr.copy()
    scaled.vec[3] = [3 * x for x in scaled.vec[3]]   # B scaled by a constant: beta' = 3 beta, but beta_g2 is still [beta]
    scaled = scaled.copy()
    assert model.mask(scaled, seed) == model.BETA_G2
    scaled.beta2 = 3 * 7
    assert model.mask(scaled, seed) == 0
    zero = tr.copy()
    zero.vec[2][2] = 0   # an identity inside A: consumed by P(A) and Q(A)
    assert model.mask(zero, seed) & model.ALPHA


def test_entry_points_declared_bound_and_exported():
    """what this feature adds to the boundary; that EVERY declared entry point is bound, exported, in ffi.rs and in the
    version script is tests/test_abi_cpu.py::test_every_entry_point_is_declared_bound_and_exported"""
    header = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    from bellman_amd import _lib

    ffi = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
    assert "bh_ptau_report;" in header and "pub struct BhPtauReport" in ffi
    assert re.search(r"#define BH_ERR_INVALID_TRANSCRIPT 10\b", header) and "BH_ERR_INVALID_TRANSCRIPT: c_int = 10" in ffi
    assert re.search(r"SEED MUST BE CHOSEN AFTER THE TRANSCRIPT IS FIXED", header)
    assert re.search(r"NOT COVERED", header)
    test_header = open(os.path.join(ROOT, "include", "bellman_hip_test.h")).read()
    for name in ("bh_test_ptau_rlc_host", "bh_test_ptau_rlc_dev", "bh_test_ptau_sums"):
        assert re.search(r"\b%s\(" % name, test_header) and name in _lib.TEST_EXPORTS, name
