"""Proofs of several verifying keys in one call, without a GPU: the new entry points in the header, the ctypes table, the
library and the generated Rust declarations (and nowhere in the test header), the hooks of the key-aware kernels in the test
header, and the exponent model tests/models/verify_keys_model.py that the GPU tests of the batch check rest on, against
real pairings of oracle/pyref."""

import os
import re
import subprocess

from oracle.pyref import pairing
from tests import group_model as gm
from tests.models import pairing_stage_model as psm
from tests.models import verify_keys_model as vkm

Q = psm.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "bh_groth16_pvk_set_create": "int", "bh_groth16_pvk_set_len": "size_t", "bh_groth16_pvk_set_release": "void",
    "bh_groth16_verify_each_keys": "int", "bh_groth16_verify_each_keys_compressed": "int",
    "bh_groth16_batch_verify_keys": "int", "bh_groth16_batch_verify_keys_compressed": "int",
}
HOOKS = ("bh_test_pairing_ic_accumulate_keys_dev", "bh_test_pairing_miller3_keys_dev", "bh_test_pairing_fold3_const_keys_dev",
         "bh_test_pairing_colsum_keys_dev", "bh_test_pairing_g1_mul_keys_dev", "bh_test_pairing_miller_keys_dev")


def test_entry_points_in_header_ctypes_library_and_rust():
    import bellman_amd
    from bellman_amd import _lib, verifier

    header = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    test_header = open(os.path.join(ROOT, "include", "bellman_hip_test.h")).read()
    ffi = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret in ENTRY_POINTS.items():
        assert re.search(r"^%s\s+%s\(" % (ret, name), header, flags=re.M), name
        assert name in _lib.EXPORTS and name not in _lib.TEST_EXPORTS, name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert "pub fn %s(" % name in ffi, name
        assert name not in test_header, name
    assert re.search(r"#define BH_PVK_SET_MAX_KEYS 64\b", header)
    assert "typedef struct bh_pvk_set bh_pvk_set;" in header and "pub struct BhPvkSet" in ffi
    assert "pvks: *const *const BhPvk" in ffi
    # the seed rule, across keys
    assert re.search(r"DRAWN AFTER THE BATCH IS FIXED", header) and re.search(r"DIFFERENT keys", header)
    test_syms = subprocess.run(["nm", "-D", "--defined-only", _lib.TEST_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in HOOKS:
        assert re.search(r"\bint %s\(" % name, test_header) and name in _lib.TEST_EXPORTS, name
        assert name not in header and name not in _lib.EXPORTS, name
        assert re.search(r" T %s$" % name, test_syms, flags=re.M), name
    for name in ("KeySet", "MultiVerifier", "verify_each_keys"):
        assert getattr(bellman_amd, name) is getattr(verifier, name), name
    for name in ("queue", "verify", "verify_multicore", "verify_each", "find_invalid"):
        assert callable(getattr(verifier.MultiVerifier, name)) and callable(getattr(verifier.Verifier, name)), name


def test_exponent_is_zero_for_a_proof_and_minus_t_d_after_a_shift_of_c():
    for n_inputs, tag in ((0, "cpu 0"), (1, "cpu 1"), (5, "cpu 5")):
        key = psm.ScalarKey(n_inputs, tag)
        rnd = psm.rng("exponent " + tag)
        inputs = [rnd.randrange(Q) for _ in range(n_inputs)]
        proof, (r, s, c) = vkm.proof_with_logs(key, inputs)
        assert proof == (gm.mul(1, gm.GEN[1], r), gm.mul(2, gm.GEN[2], s), gm.mul(1, gm.GEN[1], c))
        assert vkm.exponent(key, (r, s, c), inputs) == 0
        t = rnd.randrange(1, Q)
        assert vkm.shift_c(proof, t) == (proof[0], proof[1], gm.mul(1, gm.GEN[1], (c + t) % Q))
        assert vkm.exponent(key, (r, s, c + t), inputs) == -t * key.d % Q != 0
        if n_inputs:
            wrong = [(inputs[0] + 1) % Q] + inputs[1:]
            assert vkm.exponent(key, (r, s, c), wrong) == -key.c[1] * key.g % Q


def _equation_holds(key, proof, inputs):
    """e(A, B) e(acc, -gamma) e(C, -delta) e(-alpha, beta) == 1 by the Miller loop and final exponentiation of oracle/pyref"""
    acc = psm.ic_accumulate(key.ic[0], key.ic[1:], inputs)
    return pairing.pairing_product_is_one([(proof[0], proof[1]), (acc, gm.neg(2, key.gamma)), (proof[2], gm.neg(2, key.delta)),
                                           (gm.neg(1, key.alpha), key.beta)])


def test_exponent_model_equals_real_pairings():
    key = psm.ScalarKey(1, "cpu pairing")
    proof, logs = vkm.proof_with_logs(key, [7])
    assert vkm.exponent(key, logs, [7]) == 0 and _equation_holds(key, proof, [7])
    assert vkm.exponent(key, logs, [8]) != 0 and not _equation_holds(key, proof, [8])
    assert not _equation_holds(key, vkm.shift_c(proof, 5), [7])


def test_cancelling_shift_makes_the_batch_exponent_zero_but_no_key_alone():
    k1, k2 = psm.ScalarKey(1, "cpu cancel 1"), psm.ScalarKey(2, "cpu cancel 2")
    z1, z2, t1 = 0x1234567, 0x7654321, 0xABCDEF
    t2 = vkm.cancelling_shift(k1, z1, t1, k2, z2)
    e1, e2 = -t1 * k1.d % Q, -t2 * k2.d % Q          # (the exponents after the shifts, pinned above)
    assert e1 and e2
    assert vkm.batch_exponent([(z1, e1), (z2, e2), (99, 0)]) == 0
    assert vkm.batch_exponent([(z1, e1)]) != 0 and vkm.batch_exponent([(z2, e2)]) != 0
    assert vkm.batch_exponent([(z1, e1), (z2 + 1, e2)]) != 0


def test_grouping_is_a_stable_sort_into_blocks_of_one_key():
    key_of = [2, 0, 2, 1, 2, 0] + [1] * 130
    perm, segs, blocks = vkm.group_rows(key_of, [0, 3, 16, 5])
    assert perm[:2] == [1, 5] and perm[2] == 3 and perm[-3:] == [0, 2, 4] and sorted(perm) == list(range(len(key_of)))
    assert segs == [(0, 2, 0), (2, 131, 0), (133, 3, 393), (136, 0, 441)]
    assert blocks == [(0, 0, 2, 0), (1, 2, 64, 0), (1, 66, 64, 192), (1, 130, 3, 384), (2, 133, 3, 393)]
