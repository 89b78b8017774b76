"""The ceremony-step check without a GPU: the exponent model (tests/models/phase2_model.py) against real pairings of
oracle/pyref, the same-ratio rule, the host build of the comparison kernel's per-record predicate
(csrc/bases_compare.cuh through bh_test_records_differ_host) against numpy, the coefficient tags, and the new entry points
in the header, the ctypes table, the library and the generated Rust declarations."""

import ctypes
import os
import re

import numpy as np
import pytest

from oracle.pyref import bls12_381 as bls
from oracle.pyref import pairing
from tests.models import phase2_model as model
from tests.models import ptau_verify_model as ptau

Q = bls.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("bh_bases_first_difference", "bh_pairing_same_ratio_each", "bh_groth16_params_verify_step")
SEED = bytes(range(32))


def _g1(k):
    return bls.G1.mul(bls.G1.gen, k % Q) if k % Q else None


def _g2(k):
    return bls.G2.mul(bls.G2.gen, k % Q) if k % Q else None


def _pairing_says(a, b, c, d):
    """e([a]G1, [b]G2) == e([c]G1, [d]G2) by the Miller loop and final exponentiation of oracle/pyref"""
    return pairing.pairing_product_is_one([(_g1(a), _g2(b)), (bls.G1.neg(_g1(c)) if c % Q else None, _g2(d))])


def _params():
    return model.Params(alpha_g1=11, beta_g1=13, beta_g2=13, gamma_g2=17, delta_g1=19, delta_g2=19, ic=(23, 29),
                        h=(31, 37, 41), l=(43, 47), a=(53, 59), b_g1=(61, 67), b_g2=(61, 67))


def _mask_by_pairings(before, after, seed):
    """the three equations of a step evaluated with real pairings over the model's sums"""
    s = model.sums(before, after, seed)
    got = 0
    if not _pairing_says(after.delta_g1, before.delta_g2, before.delta_g1, after.delta_g2):
        got |= model.DELTA
    if not _pairing_says(s[0][0], before.delta_g2, s[1][0], after.delta_g2):
        got |= model.H
    if not _pairing_says(s[2][0], before.delta_g2, s[3][0], after.delta_g2):
        got |= model.L
    return got


@pytest.mark.parametrize("fault", ["honest", "delta", "h", "l"])
def test_exponent_model_equals_real_pairings(fault):
    before = _params()
    after = model.rescale_delta(before, 0xD1CE)
    want = 0
    if fault == "delta":   # delta_g1 scaled by another factor than delta_g2: H and L still relate to delta_g2
        after, want = after._replace(delta_g1=after.delta_g1 + 1), model.DELTA
    elif fault == "h":
        after, want = after._replace(h=after.h[:2] + (after.h[2] + 1,)), model.H
    elif fault == "l":
        after, want = after._replace(l=(after.l[0] + 1,) + after.l[1:]), model.L
    assert model.step(before, after, SEED) == (want, 0, 0)
    assert _mask_by_pairings(before, after, SEED) == want


def test_same_ratio_rule_equals_real_pairings():
    rows = [(3, 15, 7, 35), (3, 15, 7, 36), (3, 0, 7, 35)]   # equal ratios, unequal, an identity
    assert model.same_ratio(rows) == [model.OK, model.INVALID_TRANSCRIPT, model.POINT_AT_INFINITY]
    for (a, b, A, B), verdict in zip(rows[:2], model.same_ratio(rows)):
        assert _pairing_says(a, B, b, A) == (verdict == model.OK)
    # the identity row: the product of pairings is NOT 1, but even an identity on both sides, where it is, proves nothing
    assert model.same_ratio([(0, 0, 7, 35), (3, 15, 0, 0), (3, model.OFF, 7, 35), (0, model.OFF, 7, 35)]) == [
        model.POINT_AT_INFINITY, model.POINT_AT_INFINITY, model.INVALID_POINT, model.POINT_AT_INFINITY]


def test_model_masks_vectors_and_indices():
    before = _params()
    after = model.rescale_delta(before, 5)
    assert model.step(before, after, SEED) == (0, 0, 0)
    assert model.step(before, before, SEED) == (0, 0, 0)   # d = 1
    assert model.step(before, model.rescale_delta(after, 7), SEED) == (0, 0, 0)   # two steps composed
    assert model.step(before, after._replace(ic=after.ic + (1,)), SEED) == (model.SHAPE, 0, 0)
    assert model.step(before, after._replace(h=after.h[:-1]), SEED) == (model.SHAPE, 0, 0)
    assert model.step(before, after._replace(delta_g2=0), SEED) == (model.HEAD, 0, 0)
    assert model.step(before, after._replace(delta_g1=model.OFF), SEED) == (model.HEAD, 0, 0)
    assert model.step(before, after._replace(gamma_g2=1), SEED) == (model.KEY, 0, 3)
    assert model.step(before, after._replace(ic=(23, 30)), SEED) == (model.KEY, 0, 5)
    assert model.step(before, after._replace(b_g1=(61, 68)), SEED) == (model.B_G1, 2, 1)
    both = after._replace(a=(54, 59), b_g2=(62, 67), beta_g1=1)
    assert model.step(before, both, SEED) == (model.KEY | model.A | model.B_G2, 0, 1)   # the first finding is named
    assert model.step(before, after._replace(a=(54, 59), b_g2=(62, 67)), SEED) == (model.A | model.B_G2, 1, 0)
    assert model.step(before, after._replace(h=(after.h[0], 0, after.h[2])), SEED) == (model.H, 0, 0)   # an identity inside h'
    other = model.rescale_delta(before, 6)
    assert model.step(before, after._replace(l=other.l), SEED) == (model.L, 0, 0)   # l scaled by another factor than h
    assert model.step(before, after._replace(delta_g1=other.delta_g1, delta_g2=other.delta_g2), SEED) == (model.H | model.L, 0, 0)
    empty = before._replace(h=())
    assert model.step(empty, model.rescale_delta(empty, 5), SEED) == (0, 0, 0)   # an empty query: vacuous
    assert model.step(before, after, SEED, bad_points=(5, 1)) == (model.POINTS, 5, 1)
    assert model.validation_finding(after._replace(l=(after.l[0], 0))) == (5, 1)
    # a chain of contributions: a wrong [d]s, a wrong [d]r, a broken link
    ds, chal = [3, 5, 7], [101, 103, 107]
    deltas = [19, 19 * 3, 19 * 15, 19 * 105]
    good = [model.contribution(deltas[j], ds[j], 1000 + j, chal[j]) for j in range(3)]
    assert [c[0] for c in good] == deltas[1:]
    assert model.contributions(19, good, chal) == [0, 0, 0]
    for j in range(3):
        d_after, s, d_s, d_r = good[j]
        assert model.contributions(19, good[:j] + [(d_after, s, d_s + 1, d_r)] + good[j + 1:], chal)[j] == model.INVALID_TRANSCRIPT
        assert model.contributions(19, good[:j] + [(d_after, s, d_s, d_r + 1)] + good[j + 1:], chal)[j] == model.INVALID_TRANSCRIPT
        broken = model.contributions(19, good[:j] + [(d_after + 1, s, d_s, d_r)] + good[j + 1:], chal)
        assert [k for k, v in enumerate(broken) if v] == [k for k in (j, j + 1) if k < 3]   # both links of delta_after break


def test_tags_4_and_5_give_streams_disjoint_from_the_transcript_tags():
    streams = [ptau.coefficients(SEED, v, 64) for v in range(6)]
    assert model.TAG_H == 4 and model.TAG_L == 5
    for tag in (4, 5):
        others = set().union(*[set(s) for v, s in enumerate(streams) if v != tag])
        assert not set(streams[tag]) & others
        assert len(set(streams[tag])) == 64


@pytest.mark.parametrize("group,words", [(1, 12), (2, 24)])
def test_host_predicate_equals_numpy(group, words):
    from bellman_amd import _lib

    lib = _lib.load()
    rnd = np.random.default_rng(group)
    n = 131
    a = rnd.integers(0, 1 << 63, size=(n, words), dtype=np.uint64)
    b = a.copy()
    b[0, 0] ^= 1                                 # the first bit of the first record
    b[5, words - 1] ^= np.uint64(1 << 63)        # the last bit of a record: only its last 8 bytes differ
    b[64] = 0                                    # the identity against a point
    a[70] = 0                                    # ... and the other way round
    a[71] = b[71] = 0                            # identity against identity: equal
    for w in range(words):                       # one word at a time: every 16-byte vector and both of its halves
        b[80 + w, w] ^= np.uint64(1 << (w % 64))
    b[n - 1, words // 2] += np.uint64(1)
    want = (a != b).any(axis=1)
    assert want.sum() == 5 + words and not want[71]
    # 16-byte aligned copies (the predicate reads 16-byte vectors)
    buf_a, buf_b = np.zeros(n * words + 2, np.uint64), np.zeros(n * words + 2, np.uint64)
    va = buf_a[(-buf_a.ctypes.data % 16) // 8:][:n * words].reshape(n, words)
    vb = buf_b[(-buf_b.ctypes.data % 16) // 8:][:n * words].reshape(n, words)
    va[:], vb[:] = a, b
    out = np.full(n + 1, 7, dtype=np.uint8)
    assert lib.bh_test_records_differ_host(group, va.ctypes.data_as(ctypes.c_void_p), vb.ctypes.data_as(ctypes.c_void_p), n,
                                           out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert out[n] == 7 and (out[:n] == want.astype(np.uint8)).all()
    assert lib.bh_test_records_differ_host(group, ctypes.c_void_p(va.ctypes.data + 8), vb.ctypes.data_as(ctypes.c_void_p), 1,
                                           out.ctypes.data_as(ctypes.c_void_p)) == -2   # not 16-byte aligned
    shape = (ctypes.c_uint32 * 2)()
    lib.bh_test_compare_shape(shape)
    assert shape[0] == 256 and shape[0] % 64 == 0 and shape[1] >= 1


def test_entry_points_declared_bound_and_exported():
    """what this feature adds to the boundary; that EVERY declared entry point is bound, exported, in ffi.rs and in the
    version script is tests/test_abi_cpu.py::test_every_entry_point_is_declared_bound_and_exported"""
    header = open(os.path.join(ROOT, "include", "bellman_hip.h")).read()
    from bellman_amd import _lib
    from bellman_amd import ceremony, groth16

    ffi = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
    assert "bh_params_step_report;" in header and "pub struct BhParamsStepReport" in ffi
    for bit, name in enumerate(("SHAPE", "HEAD", "KEY", "A", "B_G1", "B_G2", "DELTA", "H", "L", "POINTS")):
        assert re.search(r"#define BH_STEP_FAILED_%s 0x%03xu\b" % (name, 1 << bit), header), name
        assert getattr(groth16, "STEP_FAILED_" + name) == getattr(model, name) == 1 << bit
    assert ctypes.sizeof(groth16.ParamsStepReport) == 16
    assert re.search(r"DRAWN\s+\*?\s*AFTER `after` IS FIXED", header) and "d = 1" in header
    assert "resident form of every handle this library makes is the reduced" in header
    test_header = open(os.path.join(ROOT, "include", "bellman_hip_test.h")).read()
    for name in ("bh_test_phase2_sums", "bh_test_records_differ_host", "bh_test_compare_shape"):
        assert re.search(r"\b%s\(" % name, test_header) and name in _lib.TEST_EXPORTS, name
    for name in ("bases_first_difference", "same_ratio_each", "contribute", "verify_contributions", "tau_is_root_of_unity"):
        assert callable(getattr(ceremony, name)), name
