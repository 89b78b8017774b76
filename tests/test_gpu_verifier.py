"""Groth16 verification on the device (bellman_amd/csrc/pairing.hip): pairings against oracle/pyref and the host build of the
same arithmetic, verify_proof (groth16/src/verifier.rs:23-58) and batch::Verifier (groth16/src/verifier/batch.rs)."""

import ctypes
import os
import random
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import cref  # noqa: E402
from oracle.cengine import CBls12  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from oracle.pyref import pairing as pyp  # noqa: E402
from tests import circuits  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401
from tests.test_verifier_cpu import g1_rec, g2_rec, gt_from_bytes, host_pairings, pyref_pairing_cubed  # noqa: E402

pytestmark = pytest.mark.gpu
Q = bls.Q


def _recs(group, pts):
    w = 12 if group == 1 else 24
    return np.frombuffer(b"".join(bytes(p) for p in pts), dtype=np.uint64).reshape(-1, w)


def dev_pairings(worker, pairs):
    from bellman_amd import _lib

    lib = _lib.load()
    a = b"".join(g1_rec(p) for p, _ in pairs)
    b = b"".join(g2_rec(q) for _, q in pairs)
    out = ctypes.create_string_buffer(576 * len(pairs))
    assert lib.bh_test_pairing(worker.ctx, len(pairs), a, b, out) == 0
    return [gt_from_bytes(out.raw, i) for i in range(len(pairs))]


def test_pairing_parity_with_pyref(worker):
    from bellman_amd import _lib

    lib = _lib.load()
    rnd = random.Random(11)
    g1, g2 = bls.G1.gen, bls.G2.gen
    pairs = [(g1, g2), (bls.G1.mul(g1, rnd.randrange(1, Q)), bls.G2.mul(g2, rnd.randrange(1, Q))), (None, g2), (g1, None),
             (bls.G1.mul(g1, rnd.randrange(1, Q)), g2)]
    got = dev_pairings(worker, pairs)
    for i in (0, 1, 4):
        assert got[i] == pyref_pairing_cubed(*pairs[i])
    assert got[2] == pyp.F12_ONE and got[3] == pyp.F12_ONE
    assert got == host_pairings(lib, pairs)


def test_pairing_bilinear_256(worker):
    from bellman_amd import _lib

    lib = _lib.load()
    rnd = random.Random(12)
    n = 256
    g1 = bytes(g1_rec(bls.G1.gen))
    g2 = bytes(g2_rec(bls.G2.gen))

    def mul(group, base, k):
        out = ctypes.create_string_buffer(96 if group == 1 else 192)
        lib.bh_test_point_mul_host(group, out, base, k.to_bytes(32, "little"))
        return out.raw

    lhs_a, lhs_b, rhs_a, rhs_b, neg_a, ps = [], [], [], [], [], []
    for _ in range(n):
        a, b, s, t = (rnd.randrange(1, Q) for _ in range(4))
        p, q = mul(1, g1, s), mul(2, g2, t)
        lhs_a.append(mul(1, p, a))
        lhs_b.append(mul(2, q, b))
        rhs_a.append(mul(1, p, a * b % Q))
        rhs_b.append(q)
        neg_a.append(mul(1, p, Q - 1))
        ps.append(p)
    out1, out2, out3 = (ctypes.create_string_buffer(576 * n) for _ in range(3))
    assert lib.bh_test_pairing(worker.ctx, n, b"".join(lhs_a), b"".join(lhs_b), out1) == 0
    assert lib.bh_test_pairing(worker.ctx, n, b"".join(rhs_a), b"".join(rhs_b), out2) == 0
    assert out1.raw == out2.raw
    # e(-P, Q) = e(P, Q)^-1: the conjugate (w^k coefficients times (-1)^k) in the cyclotomic subgroup
    assert lib.bh_test_pairing(worker.ctx, n, b"".join(neg_a), b"".join(rhs_b), out3) == 0
    out4 = ctypes.create_string_buffer(576 * n)
    assert lib.bh_test_pairing(worker.ctx, n, b"".join(ps), b"".join(rhs_b), out4) == 0
    for i in range(0, n, 17):
        e, e_neg = gt_from_bytes(out4.raw, i), gt_from_bytes(out3.raw, i)
        assert pyp.f12_mul(e, e_neg) == pyp.F12_ONE


# ---- verify_proof -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mimc(worker):
    """generate_parameters for MiMC-322 and four proofs of distinct preimages (groth16/tests/mimc.rs:38-101)"""
    from bellman_amd import groth16 as pg
    from bellman_amd import verifier

    rnd = random.Random(2718)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    r1cs = pg.R1CS.from_demo(worker, 0, circuits.MIMC_ROUNDS, 0, cons)
    g1, g2 = _recs(1, [CBls12.G1.gen])[0], _recs(2, [CBls12.G2.gen])[0]
    params = pg.Parameters.generate(worker, r1cs, g1, g2, *[rnd.randrange(1, Q) for _ in range(5)])
    proofs, images = [], []
    for _ in range(4):
        xl, xr = rnd.randrange(Q), rnd.randrange(Q)
        images.append(circuits.mimc_hash(xl, xr, cons))
        proofs.append(pg.create_random_proof(circuits.mimc_circuit(xl, xr, cons), params, rng=rnd, r1cs=r1cs))
    pvk = verifier.prepare_verifying_key(params)
    yield dict(params=params, pvk=pvk, proofs=proofs, images=images, cons=cons)
    pvk.release()


def _copy(proof):
    from bellman_amd import groth16 as pg

    return pg.Proof(np.concatenate([proof.a, proof.b, proof.c]).astype(np.uint64))


def _pyref_vk_proof(params, proof):
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    vk = dict(alpha_g1=cref.g1_to_py(alpha_g1)[0], beta_g2=cref.g2_to_py(beta_g2)[0], gamma_g2=cref.g2_to_py(gamma_g2)[0],
              delta_g2=cref.g2_to_py(delta_g2)[0], ic=cref.g1_to_py(ic))
    return vk, (cref.g1_to_py(proof.a)[0], cref.g2_to_py(proof.b)[0], cref.g1_to_py(proof.c)[0])


def _g1_arr(pt):
    return np.frombuffer(g1_rec(pt), dtype=np.uint64).copy()


def test_verify_proof_mimc(mimc):
    from bellman_amd import InvalidPoint, InvalidProof, InvalidVerifyingKey, verify_proof

    pvk, proofs, images = mimc["pvk"], mimc["proofs"], mimc["images"]
    for pr, im in zip(proofs, images):
        verify_proof(pvk, pr, [im])
    p0 = proofs[0]
    with pytest.raises(InvalidProof):
        verify_proof(pvk, p0, [(images[0] + 1) % Q])
    c2 = _copy(p0)
    c2.c = _g1_arr(bls.G1.double(cref.g1_to_py(p0.c)[0]))
    with pytest.raises(InvalidProof):
        verify_proof(pvk, c2, [images[0]])
    sw = _copy(p0)
    sw.a = proofs[1].a.copy()                # A of one proof with B and C of another
    with pytest.raises(InvalidProof):
        verify_proof(pvk, sw, [images[0]])
    ai = _copy(p0)
    ai.a = np.zeros(12, dtype=np.uint64)
    with pytest.raises(InvalidProof):
        verify_proof(pvk, ai, [images[0]])
    with pytest.raises(InvalidVerifyingKey):
        verify_proof(pvk, p0, [images[0], 1])
    with pytest.raises(InvalidVerifyingKey):
        verify_proof(pvk, p0, [])
    off = _copy(p0)
    off.a = off.a.copy()
    off.a[0] ^= np.uint64(1)
    with pytest.raises(InvalidPoint):
        verify_proof(pvk, off, [images[0]])
    # three of the cases against the oracle's restatement of verify_proof
    for pr, ok in ((p0, True), (c2, False), (sw, False)):
        vk, pp = _pyref_vk_proof(mimc["params"], pr)
        assert pyp.verify_proof(vk, pp, [images[0]]) == ok


def test_verify_proof_without_public_inputs(worker, mimc):
    """ic of length 1: the MiMC key with its one input folded into ic_0 verifies the same proof with no inputs"""
    from bellman_amd import InvalidProof, verifier

    params, p0 = mimc["params"], mimc["proofs"][0]
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    ic_py = cref.g1_to_py(ic)
    folded = bls.G1.add(ic_py[0], bls.G1.mul(ic_py[1], mimc["images"][0]))
    pvk0 = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, _g1_arr(folded).reshape(1, 12))
    assert pvk0.n_inputs == 0
    verifier.verify_proof(pvk0, p0, [])
    with pytest.raises(InvalidProof):
        verifier.verify_proof(pvk0, mimc["proofs"][1], [])


# ---- batch::Verifier -------------------------------------------------------------------------------------------------
def _rerandomised(worker, mimc, n, seed):
    """n valid proofs: (A / theta, B theta, C) of the fixture's four proofs, two fixed-base calls per group"""
    from bellman_amd import _lib
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    rnd = random.Random(seed)
    out = []
    for k, (base, im) in enumerate(zip(mimc["proofs"], mimc["images"])):
        m = n // 4 + (1 if k < n % 4 else 0)
        if not m:
            continue
        th = [rnd.randrange(1, Q) for _ in range(m)]
        sc = [np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()
              for vals in ([pow(t, -1, Q) for t in th], th)]
        res = []
        for group, pt, s in ((1, base.a, sc[0]), (2, base.b, sc[1])):
            w = 12 if group == 1 else 24
            ds, do = worker.alloc(m * 32), worker.alloc(m * 8 * w)
            worker.upload(ds, s)
            assert lib.bh_fixed_base_mul_dev(worker.ctx, group, np.ascontiguousarray(pt).ctypes.data_as(ctypes.c_void_p), ds, m, 0,
                                             do, None) == 0
            worker.synchronize()
            h = np.zeros((m, w), dtype=np.uint64)
            worker.download(h, do)
            worker.free(ds)
            worker.free(do)
            res.append(h)
        for j in range(m):
            out.append((pg.Proof(np.concatenate([res[0][j], res[1][j], base.c])), [im]))
    return out


@pytest.fixture(scope="module")
def many(worker, mimc):
    return _rerandomised(worker, mimc, 16384 + 1000, 99)


def _batch(items):
    from bellman_amd import Verifier

    v = Verifier()
    for it in items:
        v.queue(it)
    return v


def test_batch_sizes_pass(mimc, many):
    pvk = mimc["pvk"]
    rnd = random.Random(5)
    for n in (1, 2, 7, 64, 1024, 16384):
        _batch(many[:n]).verify(rnd, pvk)
    _batch([]).verify(rnd, pvk)
    _batch(many[:3]).verify_multicore(pvk)


def test_batch_corruption_anywhere_fails(mimc, many):
    from bellman_amd import InvalidProof

    pvk = mimc["pvk"]
    rnd = random.Random(6)
    items = list(many[:1024])
    for pos in (0, 511, 1023):
        bad = list(items)
        pr, ins = bad[pos]
        bad[pos] = (pr, [(ins[0] + 1) % Q])
        with pytest.raises(InvalidProof):
            _batch(bad).verify(rnd, pvk)


def test_batch_argument_errors(mimc, many):
    from bellman_amd import InvalidVerifyingKey
    from bellman_amd import _lib

    pvk = mimc["pvk"]
    items = list(many[:8])
    items[5] = (items[5][0], [])
    with pytest.raises(InvalidVerifyingKey):
        _batch(items).verify(random.Random(1), pvk)
    # a zero z: INVALID_ARG
    lib = _lib.load()
    from bellman_amd.verifier import _fr_bytes, _proof_bytes

    pr = b"".join(_proof_bytes(p) for p, _ in many[:2])
    ins = _fr_bytes([many[0][1][0], many[1][1][0]])
    assert lib.bh_groth16_batch_verify(pvk._h, pr, 2, ins, 1, 0, _fr_bytes([3, 0])) == -2
    assert lib.bh_groth16_batch_verify(pvk._h, pr, 2, ins, 1, 0, _fr_bytes([3, 5])) == 0


def test_batch_equals_and_of_verify_single(mimc, many):
    from bellman_amd import InvalidProof
    from bellman_amd.verifier import Item

    pvk = mimc["pvk"]
    rnd = random.Random(9)
    items = [Item(p, i) for p, i in many[:32]]
    for k in (3, 17):
        items[k] = Item(items[k].proof, [(items[k].inputs[0] + k) % Q])
    singles = []
    for it in items:
        try:
            it.verify_single(pvk)
            singles.append(True)
        except InvalidProof:
            singles.append(False)
    assert singles.count(False) == 2
    with pytest.raises(InvalidProof):
        _batch(items).verify(rnd, pvk)
    good = [it for it, ok in zip(items, singles) if ok]
    _batch(good).verify(rnd, pvk)


def test_batch_over_one_chunk(mimc, many):
    from bellman_amd import InvalidProof

    pvk = mimc["pvk"]
    rnd = random.Random(10)
    _batch(many).verify(rnd, pvk)          # 17384 proofs: two chunks
    bad = list(many)
    pr, ins = bad[-3]
    bad[-3] = (pr, [(ins[0] + 1) % Q])      # in the second chunk
    with pytest.raises(InvalidProof):
        _batch(bad).verify(rnd, pvk)
    _batch(many[:16384]).verify(rnd, pvk)
    _batch(many[16384:]).verify(rnd, pvk)


def test_batch_threads_beside_a_proof(worker, mimc, many):
    from bellman_amd import InvalidProof
    from bellman_amd import groth16 as pg

    pvk = mimc["pvk"]
    results = [None] * 4

    def run(k):
        rnd = random.Random(100 + k)
        items = list(many[k * 200:(k + 1) * 200])
        want_ok = k % 2 == 0
        if not want_ok:
            pr, ins = items[7]
            items[7] = (pr, [(ins[0] + 1) % Q])
        try:
            _batch(items).verify(rnd, pvk)
            results[k] = want_ok
        except InvalidProof:
            results[k] = not want_ok

    rnd = random.Random(77)
    cons_params = mimc["params"]
    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    xl, xr = rnd.randrange(Q), rnd.randrange(Q)
    cons = mimc["cons"]
    proof = pg.create_random_proof(circuits.mimc_circuit(xl, xr, cons), cons_params, rng=rnd)
    for t in threads:
        t.join()
    assert results == [True] * 4
    from bellman_amd import verify_proof

    verify_proof(pvk, proof, [circuits.mimc_hash(xl, xr, cons)])


def _mont(v):
    return (v * (1 << 256) % Q).to_bytes(32, "little")


def test_montgomery_scalars_verify_and_batch(mimc, many):
    """BH_SCALARS_MONT inputs and z for bh_groth16_verify and bh_groth16_batch_verify"""
    from bellman_amd import _lib
    from bellman_amd.verifier import _proof_bytes

    lib = _lib.load()
    pvk, p0, im = mimc["pvk"], mimc["proofs"][0], mimc["images"][0]
    assert lib.bh_groth16_verify(pvk._h, _proof_bytes(p0), _mont(im), 1, 1) == 0
    assert lib.bh_groth16_verify(pvk._h, _proof_bytes(p0), _mont(im + 1), 1, 1) == 9
    items = many[:40]
    pr = b"".join(_proof_bytes(p) for p, _ in items)
    rnd = random.Random(21)
    z = b"".join(_mont(rnd.randrange(1, Q)) for _ in items)
    assert lib.bh_groth16_batch_verify(pvk._h, pr, len(items), b"".join(_mont(i[0]) for _, i in items), 1, 1, z) == 0
    bad = [i[0] for _, i in items]
    bad[13] += 1
    assert lib.bh_groth16_batch_verify(pvk._h, pr, len(items), b"".join(_mont(v) for v in bad), 1, 1, z) == 9


def test_batch_zero_z_modulo_q_and_off_curve_point(mimc, many):
    from bellman_amd import InvalidPoint
    from bellman_amd import _lib
    from bellman_amd.verifier import _fr_bytes, _proof_bytes

    lib = _lib.load()
    pvk = mimc["pvk"]
    items = list(many[:16])
    pr = b"".join(_proof_bytes(p) for p, _ in items)
    ins = _fr_bytes([i[0] for _, i in items])
    for zero in (0, Q, 2 * Q):   # all zero in Fr: refused like z = 0 (batch.rs:117-128)
        z = b"".join(v.to_bytes(32, "little") for v in [5] * 7 + [zero] + [9] * 8)
        assert lib.bh_groth16_batch_verify(pvk._h, pr, 16, ins, 1, 0, z) == -2
    # an off-curve B (and separately A) in the middle of the batch
    for field in ("b", "a"):
        bad = list(items)
        p = _copy(bad[9][0])
        arr = getattr(p, field).copy()
        arr[0] ^= np.uint64(1)
        setattr(p, field, arr)
        bad[9] = (p, bad[9][1])
        with pytest.raises(InvalidPoint):
            _batch(bad).verify(random.Random(3), pvk)


def test_identity_ic_entry(worker, mimc, many):
    """a key whose ic_0 is the identity: ic' = [O, ic_0, ic_1] with inputs [1, x] describes the same statement; single and
    batch verification agree"""
    from bellman_amd import InvalidProof, verifier
    from bellman_amd.verifier import Item

    params = mimc["params"]
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    ic3 = np.concatenate([np.zeros((1, 12), dtype=np.uint64), ic])
    pvk3 = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, ic3)
    try:
        assert pvk3.n_inputs == 2
        items = [Item(p, [1, i[0]]) for p, i in many[:24]]
        for it in items[:4]:
            it.verify_single(pvk3)
        _batch(items).verify(random.Random(4), pvk3)
        items[6] = Item(items[6].proof, [1, items[6].inputs[1] + 1])
        with pytest.raises(InvalidProof):
            items[6].verify_single(pvk3)
        with pytest.raises(InvalidProof):
            _batch(items).verify(random.Random(4), pvk3)
    finally:
        pvk3.release()
