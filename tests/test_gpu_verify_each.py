"""Per-proof verdicts for many proofs in one call (bh_groth16_verify_each / _compressed, bellman_amd.verifier.verify_each,
Verifier.find_invalid): Item::verify_single (groth16/src/verifier/batch.rs:55-66) for every proof of a batch.  The contract
under test is one sentence per entry point: verdicts[j] is the code bh_groth16_verify (after bh_proofs_read, for bytes)
returns for proof j alone."""

import ctypes
import os
import random
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import cref  # noqa: E402
from oracle.pyref import bls12_381 as bls  # noqa: E402
from oracle.pyref import pairing as pyp  # noqa: E402
from tests import circuits, pointgen  # noqa: E402
from tests.test_gpu_groth16 import _chain_setup, worker  # noqa: E402,F401
from tests.test_gpu_proof_read import _non_residue_x, _set  # noqa: E402
from tests.test_gpu_verifier import _batch, _copy, _g1_arr, _mont, _pyref_vk_proof, _rerandomised, mimc  # noqa: E402,F401

pytestmark = pytest.mark.gpu
Q = bls.Q
OK, INVALID_POINT, AT_INFINITY, INVALID_PROOF, INVALID_KEY, INVALID_ARG = 0, 6, 7, 9, 8, -2


def _lib():
    from bellman_amd import _lib as L

    return L.load()


def _raw(v):
    """an input as 32 little-endian bytes, NOT reduced (values >= q stay as they are)"""
    return int(v).to_bytes(32, "little")


def _proof_bytes(p):
    from bellman_amd.verifier import _proof_bytes as pb

    return pb(p)


def _each(pvk, items, fmt=0, enc=_raw, n_inputs=None):
    """bh_groth16_verify_each over (proof, inputs) pairs -> (rc, verdicts, n_bad)"""
    n = len(items)
    n_in = pvk.n_inputs if n_inputs is None else n_inputs
    proofs = b"".join(_proof_bytes(p) for p, _ in items)
    ins = b"".join(enc(v) for _, i in items for v in i)
    verdicts = (ctypes.c_int32 * max(n, 1))(*([-99] * max(n, 1)))
    n_bad = ctypes.c_size_t(12345)
    rc = _lib().bh_groth16_verify_each(pvk._h, proofs or None, n, ins or None, n_in, fmt, verdicts, ctypes.byref(n_bad))
    return rc, list(verdicts)[:n], n_bad.value


def _each_bytes(pvk, items, fmt=0, enc=_raw):
    """bh_groth16_verify_each_compressed over (192 bytes, inputs) pairs -> (rc, verdicts, status, n_bad)"""
    n = len(items)
    blob = b"".join(bytes(p) for p, _ in items)
    ins = b"".join(enc(v) for _, i in items for v in i)
    verdicts = (ctypes.c_int32 * max(n, 1))(*([-99] * max(n, 1)))
    status = (ctypes.c_uint32 * max(n, 1))(*([0xDEAD] * max(n, 1)))
    n_bad = ctypes.c_size_t(12345)
    rc = _lib().bh_groth16_verify_each_compressed(pvk._h, blob or None, n, ins or None, pvk.n_inputs, fmt, verdicts, status,
                                                  ctypes.byref(n_bad))
    return rc, list(verdicts)[:n], list(status)[:n], n_bad.value


def _single(pvk, proof, inputs, fmt=0, enc=_raw):
    """bh_groth16_verify on one proof alone"""
    ins = b"".join(enc(v) for v in inputs)
    return _lib().bh_groth16_verify(pvk._h, _proof_bytes(proof), ins or None, len(inputs), fmt)


def _single_bytes(worker, pvk, data, inputs):
    """bh_proofs_read on 192 bytes alone, then bh_groth16_verify on the decoded proof -> (verdict, status word)"""
    from bellman_amd import groth16 as pg

    rec = np.zeros(48, dtype=np.uint64)
    word = (ctypes.c_uint32 * 1)()
    rc = _lib().bh_proofs_read(worker.ctx, bytes(data), 1, rec.ctypes.data_as(ctypes.c_void_p), word, None)
    if rc != 0:
        return rc, word[0]
    return _single(pvk, pg.Proof(rec), inputs), word[0]


@pytest.fixture(scope="module")
def pool(worker, mimc):  # noqa: F811
    """16 MiMC proofs with distinct public inputs (the verifier fixture's four and twelve more) and 16384 + 5 valid proofs
    rerandomised from them, interleaved so that neighbouring rows differ"""
    from bellman_amd import groth16 as pg

    rnd = random.Random(31337)
    proofs, images = list(mimc["proofs"]), list(mimc["images"])
    for _ in range(12):
        xl, xr = rnd.randrange(Q), rnd.randrange(Q)
        images.append(circuits.mimc_hash(xl, xr, mimc["cons"]))
        proofs.append(pg.create_random_proof(circuits.mimc_circuit(xl, xr, mimc["cons"]), mimc["params"], rng=rnd))
    assert len(set(images)) == 16
    n = 16384 + 5
    groups = []
    for g in range(4):
        sub = dict(proofs=proofs[4 * g:4 * g + 4], images=images[4 * g:4 * g + 4])
        groups.append(_rerandomised(worker, sub, n // 4 + (1 if g < n % 4 else 0), 500 + g))
    items = []
    for k in range(max(len(g) for g in groups)):
        for g in groups:
            if k < len(g):
                items.append(g[k])
    assert len(items) == n
    # rows of neighbours differ: shuffle once, seeded
    rnd.shuffle(items)
    return dict(items=items, proofs=proofs, images=images)


def _wrong_input(item):
    p, ins = item
    return (p, [(ins[0] + 1) % Q] + list(ins[1:]))


def _off_curve(item, field):
    p = _copy(item[0])
    arr = getattr(p, field).copy()
    arr[0] ^= np.uint64(1)
    setattr(p, field, arr)
    return (p, item[1])


def _identity(item, field):
    p = _copy(item[0])
    setattr(p, field, np.zeros(24 if field == "b" else 12, dtype=np.uint64))
    return (p, item[1])


# ---- 1. the definition -----------------------------------------------------------------------------------------------
def test_verdicts_are_verify_proof_of_every_proof(mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    rnd = random.Random(1)
    n = 1000
    items = list(pool["items"][:n])
    kinds = ["wrong input", "swapped c", "a off curve", "b off curve", "c off curve", "a identity", "b identity",
             "off curve and wrong input"]
    where = rnd.sample(range(n), 6 * len(kinds))
    want = [OK] * n
    for k, j in enumerate(where):
        kind = kinds[k % len(kinds)]
        if kind == "wrong input":
            items[j], want[j] = _wrong_input(items[j]), INVALID_PROOF
        elif kind == "swapped c":
            other = next(i for i in range(n) if not (pool["items"][i][0].c == items[j][0].c).all())
            p = _copy(items[j][0])
            p.c = pool["items"][other][0].c.copy()
            items[j], want[j] = (p, items[j][1]), INVALID_PROOF
        elif kind.endswith("off curve"):
            items[j], want[j] = _off_curve(items[j], kind[0]), INVALID_POINT
        elif kind.endswith("identity"):
            items[j], want[j] = _identity(items[j], kind[0]), INVALID_PROOF
        else:
            items[j], want[j] = _wrong_input(_off_curve(items[j], "abc"[k % 3])), INVALID_POINT
    rc, got, n_bad = _each(pvk, items)
    assert rc == OK
    assert got == want
    assert n_bad == len(where) == sum(v != 0 for v in got)
    # ... and equal to bh_groth16_verify on every corrupted proof and 32 untouched ones, each alone
    untouched = [j for j in range(n) if j not in set(where)]
    for j in where + rnd.sample(untouched, 32):
        assert _single(pvk, *items[j]) == got[j], j
    # two of them against the oracle's restatement of verify_proof
    good, bad = untouched[0], where[0]
    for j, ok in ((good, True), (bad, False)):
        vk, pp = _pyref_vk_proof(mimc["params"], items[j][0])
        assert pyp.verify_proof(vk, pp, items[j][1]) == ok
        assert (got[j] == OK) == ok


# ---- 2. row j belongs to proof j -------------------------------------------------------------------------------------
def test_input_rows_are_bound_to_their_proofs(mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    items = list(pool["items"][:12])
    i = 2
    j = next(k for k in range(3, 12) if items[k][1] != items[i][1])
    items[i], items[j] = (items[i][0], items[j][1]), (items[j][0], items[i][1])
    rc, got, n_bad = _each(pvk, items)
    assert rc == OK and n_bad == 2
    assert got == [INVALID_PROOF if k in (i, j) else OK for k in range(12)]


# ---- 3. sizes, across a chunk ----------------------------------------------------------------------------------------
def test_sizes_and_chunk_boundary(mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    for n in (0, 1, 63, 64, 65, 16384 + 5):
        items = list(pool["items"][:n])
        bad = sorted({j for j in (0, n - 1, 16383, 16384) if 0 <= j < n})
        for j in bad:
            items[j] = _wrong_input(items[j])
        rc, got, n_bad = _each(pvk, items)
        assert rc == OK, n
        assert [j for j in range(n) if got[j] != OK] == bad, n
        assert all(got[j] == INVALID_PROOF for j in bad)
        assert n_bad == len(bad) == sum(v != 0 for v in got)
    # an empty call needs no pointers
    n_bad = ctypes.c_size_t(7)
    assert _lib().bh_groth16_verify_each(pvk._h, None, 0, None, 1, 0, None, ctypes.byref(n_bad)) == OK and n_bad.value == 0
    assert _lib().bh_groth16_verify_each(pvk._h, None, 0, None, 1, 0, None, None) == OK


# ---- 4. keys and scalars ---------------------------------------------------------------------------------------------
def _key_elements(mimc):  # noqa: F811
    params = mimc["params"]
    alpha_g1, _, beta_g2, _, delta_g2 = params.vk()
    gamma_g2, ic = params.vk_ext()
    return alpha_g1, beta_g2, gamma_g2, delta_g2, ic


def test_key_without_public_inputs(worker, mimc, pool):  # noqa: F811
    from bellman_amd import verifier

    alpha_g1, beta_g2, gamma_g2, delta_g2, ic = _key_elements(mimc)
    ic_py = cref.g1_to_py(ic)
    im0 = pool["images"][0]
    folded = bls.G1.add(ic_py[0], bls.G1.mul(ic_py[1], im0))
    pvk0 = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, _g1_arr(folded).reshape(1, 12))
    try:
        items = [(p, []) for p, _ in pool["items"][:100]]
        want = [OK if ins == [im0] else INVALID_PROOF for _, ins in pool["items"][:100]]
        assert OK in want and INVALID_PROOF in want
        rc, got, n_bad = _each(pvk0, items)
        assert rc == OK and got == want and n_bad == want.count(INVALID_PROOF)
        for j in range(12):
            assert _single(pvk0, *items[j]) == got[j]
    finally:
        pvk0.release()


def test_key_with_an_identity_ic_entry(worker, mimc, pool):  # noqa: F811
    from bellman_amd import verifier

    alpha_g1, beta_g2, gamma_g2, delta_g2, ic = _key_elements(mimc)
    ic3 = np.concatenate([np.zeros((1, 12), dtype=np.uint64), ic])
    pvk3 = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, ic3)
    try:
        items = [(p, [1, i[0]]) for p, i in pool["items"][:70]]
        items[6] = (items[6][0], [1, (items[6][1][1] + 1) % Q])
        items[9] = (items[9][0], [2, items[9][1][1]])          # ic_1' = ic_0 taken twice
        items[11] = (items[11][0], [0, items[11][1][1]])        # ... and not at all
        rc, got, n_bad = _each(pvk3, items)
        assert rc == OK and n_bad == 3
        assert got == [INVALID_PROOF if j in (6, 9, 11) else OK for j in range(70)]
        for j in (0, 6, 9, 11, 12):
            assert _single(pvk3, *items[j]) == got[j]
        # an identity in the middle of ic: its input is free
        icm = np.concatenate([ic[:1], np.zeros((1, 12), dtype=np.uint64), ic[1:]])
        pvkm = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, icm)
        try:
            items = [(p, [j * 977 % Q, i[0]]) for j, (p, i) in enumerate(pool["items"][:20])]
            items[4] = (items[4][0], [5, (items[4][1][1] + 1) % Q])
            rc, got, _ = _each(pvkm, items)
            assert rc == OK and got == [INVALID_PROOF if j == 4 else OK for j in range(20)]
            assert [_single(pvkm, *items[j]) for j in (3, 4)] == [OK, INVALID_PROOF]
        finally:
            pvkm.release()
    finally:
        pvk3.release()


def _point_mul(lib, base, k):
    out = ctypes.create_string_buffer(96)
    lib.bh_test_point_mul_host(1, out, bytes(base), (k % Q).to_bytes(32, "little"))
    return np.frombuffer(out.raw, dtype=np.uint64).copy()


def test_key_with_sixteen_inputs_and_edge_scalars(worker, mimc, pool):  # noqa: F811
    """ic' = [ic_0, ic_1, s_2 ic_1, ..., s_16 ic_1]: inputs (x - sum s_k a_k, a_2, ..., a_16) describe the statement x for any
    a_k - among them 0, 1, q - 1 and, in the canonical format, values >= q"""
    from bellman_amd import verifier

    lib = _lib()
    alpha_g1, beta_g2, gamma_g2, delta_g2, ic = _key_elements(mimc)
    rnd = random.Random(4)
    s = [rnd.randrange(1, Q) for _ in range(15)]
    ic17 = np.concatenate([ic, np.stack([_point_mul(lib, ic[1].tobytes(), sk) for sk in s])])
    pvk17 = verifier.PreparedVerifyingKey.from_elements(worker, alpha_g1, beta_g2, gamma_g2, delta_g2, ic17)
    try:
        assert pvk17.n_inputs == 16
        edge = [0, 1, Q - 1]
        items, want = [], []
        for j, (p, i) in enumerate(pool["items"][:130]):
            a = [edge[rnd.randrange(3)] if rnd.random() < 0.4 else rnd.randrange(Q) for _ in range(15)]
            if j == 0:
                a = [0] * 15
            if j == 1:
                a = [1] * 15
            if j == 2:
                a = [Q - 1] * 15
            first = (i[0] - sum(sk * ak for sk, ak in zip(s, a))) % Q
            bad = j % 9 == 5
            if bad:
                a[j % 15] = (a[j % 15] + 1) % Q
            items.append((p, [first] + a))
            want.append(INVALID_PROOF if bad else OK)
        rc, got, n_bad = _each(pvk17, items)
        assert rc == OK and got == want and n_bad == want.count(INVALID_PROOF)
        for j in (0, 1, 2, 5, 14, 129):
            assert _single(pvk17, *items[j]) == got[j]
        # Montgomery scalars: the same verdicts
        rc, got_m, _ = _each(pvk17, items, fmt=1, enc=_mont)
        assert rc == OK and got_m == want
        assert _single(pvk17, *items[5], fmt=1, enc=_mont) == INVALID_PROOF
        # canonical values >= q: whatever bh_groth16_verify makes of them
        big = []
        for j, (p, ins) in enumerate(items[:24]):
            ins = list(ins)
            for k in range(16):
                if (j + k) % 3 == 0 and ins[k] + Q < 1 << 256:
                    ins[k] += Q
            if j % 5 == 1:
                ins[3] = (1 << 256) - 1 - j
            big.append((p, ins))
        assert any(v >= Q for _, ins in big for v in ins)
        rc, got_b, _ = _each(pvk17, big)
        assert rc == OK
        assert got_b == [_single(pvk17, *it) for it in big]
    finally:
        pvk17.release()


def test_one_input_edge_scalars_and_montgomery(mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    items = list(pool["items"][:40])
    for j, v in ((3, 0), (8, 1), (13, Q - 1)):
        items[j] = (items[j][0], [v])
    rc, got, _ = _each(pvk, items)
    assert rc == OK and got == [INVALID_PROOF if j in (3, 8, 13) else OK for j in range(40)]
    assert [_single(pvk, *items[j]) for j in (3, 8, 13, 14)] == [INVALID_PROOF] * 3 + [OK]
    rc, got_m, _ = _each(pvk, items, fmt=1, enc=_mont)
    assert rc == OK and got_m == got
    # x + q names the same statement in the canonical format if bh_groth16_verify says so
    over = [(p, [i[0] + Q]) for p, i in items[:10]]
    rc, got_o, _ = _each(pvk, over)
    assert rc == OK and got_o == [_single(pvk, *it) for it in over]


# ---- 5. the compressed form ------------------------------------------------------------------------------------------
def test_compressed_verdicts_and_status_words(worker, mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    items = pool["items"][:48]
    packed = [(p.write(), ins) for p, ins in items]
    inf1, inf2 = bls.g1_compress(None), bls.g2_compress(None)
    out1 = bls.g1_compress(pointgen.g1_on_curve_not_in_subgroup(3))
    out2 = bls.g2_compress(pointgen.g2_on_curve_not_in_subgroup(3))
    nonres = bytearray(_non_residue_x(1))
    nonres[0] |= 0x80
    nonres2 = bytearray(_non_residue_x(2))
    nonres2[0] |= 0x80

    def with_elem(k, elem, enc):
        return (_set(packed[k][0], 0, elem, bytes(enc)), packed[k][1])

    damaged = {
        2: with_elem(2, "a", bytes([packed[2][0][0] & 0x7F]) + packed[2][0][1:48]),   # compression flag clear
        5: with_elem(5, "c", nonres),
        8: with_elem(8, "b", nonres2),
        11: with_elem(11, "b", out2),
        14: with_elem(14, "a", out1),
        17: with_elem(17, "a", inf1),
        20: with_elem(20, "b", inf2),
        23: with_elem(23, "c", inf1),
        26: (_set(_set(packed[26][0], 0, "a", inf1), 0, "b", out2), packed[26][1]),   # a is reported: infinity
        29: (_set(_set(packed[29][0], 0, "a", out1), 0, "c", inf1), packed[29][1]),   # a is reported: invalid
        47: with_elem(47, "c", out1),
    }
    batch = list(packed)
    for k, it in damaged.items():
        batch[k] = it
        if k + 1 < len(batch):
            batch[k + 1] = _wrong_input(batch[k + 1])          # a wrong input right after every unreadable proof
    batch[40] = (batch[40][0], [0])
    batch[0] = _wrong_input(batch[0])
    rc, got, status, n_bad = _each_bytes(pvk, batch)
    assert rc == OK
    singles = [_single_bytes(worker, pvk, data, ins) for data, ins in batch]
    assert got == [v for v, _ in singles]
    assert status == [w for _, w in singles]
    assert n_bad == sum(v != 0 for v in got)
    for k in damaged:
        assert got[k] in (INVALID_POINT, AT_INFINITY) and status[k] != 0
        if k + 1 < len(batch):
            assert got[k + 1] == INVALID_PROOF and status[k + 1] == 0     # the proofs after a bad one are still judged
    assert [got[k] for k in (17, 20, 23, 26, 29)] == [AT_INFINITY] * 4 + [INVALID_POINT]
    assert got[0] == INVALID_PROOF and got[40] == INVALID_PROOF and got[41] == OK and got[44] == OK
    # status is optional; so is n_bad
    verdicts = (ctypes.c_int32 * len(batch))()
    blob = b"".join(d for d, _ in batch)
    ins = b"".join(_raw(v) for _, i in batch for v in i)
    assert _lib().bh_groth16_verify_each_compressed(pvk._h, blob, len(batch), ins, 1, 0, verdicts, None, None) == OK
    assert list(verdicts) == got
    assert _lib().bh_groth16_verify_each_compressed(pvk._h, None, 0, None, 1, 0, None, None, None) == OK


# ---- 6. agreement with the batch verifier; the Python API ---------------------------------------------------------------
def test_agreement_with_the_batch_and_find_invalid(worker, mimc, pool):  # noqa: F811
    import bellman_amd
    from bellman_amd import InvalidPoint, InvalidProof, InvalidVerifyingKey, PointAtInfinity, verifier

    pvk = mimc["pvk"]
    lib = _lib()
    base = pool["items"][:96]
    for seed, n_bad in ((1, 0), (2, 1), (3, 5), (4, 0), (5, 17)):
        rnd = random.Random(seed)
        items = list(base)
        bad = sorted(rnd.sample(range(len(items)), n_bad))
        for j in bad:
            items[j] = _wrong_input(items[j]) if rnd.random() < 0.7 else _identity(items[j], "a")
        rc, got, nb = _each(pvk, items)
        assert rc == OK and [j for j, v in enumerate(got) if v] == bad and nb == n_bad
        z = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in items)
        brc = lib.bh_groth16_batch_verify(pvk._h, b"".join(_proof_bytes(p) for p, _ in items), len(items),
                                          b"".join(_raw(i[0]) for _, i in items), 1, 0, z)
        assert (brc == OK) == (not any(got))
        v = _batch(items)
        assert v.find_invalid(rnd, pvk) == bad
    # the Python API: None or the exception verify_single would raise, as an instance
    items = list(base[:24])
    items[3] = _wrong_input(items[3])
    items[7] = _off_curve(items[7], "b")
    res = verifier.verify_each(pvk, items)
    assert bellman_amd.verify_each is verifier.verify_each
    assert [type(e) for e in res] == [InvalidProof if j == 3 else InvalidPoint if j == 7 else type(None) for j in range(24)]
    for j in (3, 7):
        with pytest.raises(type(res[j])):
            verifier.Item(*items[j]).verify_single(pvk)
    assert _batch(items).verify_each(pvk)[3].__class__ is InvalidProof
    assert verifier.verify_each(pvk, []) == [] and _batch([]).find_invalid(random.Random(1), pvk) == []
    # bytes only: the compressed entry point; mixed: the byte items are read first, a read error is that item's entry
    packed = [(p.write(), ins) for p, ins in base[:24]]
    packed[3] = _wrong_input(packed[3])
    packed[9] = (_set(packed[9][0], 0, "a", bls.g1_compress(None)), packed[9][1])
    packed[12] = (_set(packed[12][0], 0, "b", bls.g2_compress(pointgen.g2_on_curve_not_in_subgroup(3))), packed[12][1])
    kinds = {3: InvalidProof, 9: PointAtInfinity, 12: InvalidPoint}
    res = verifier.verify_each(pvk, packed)
    assert [type(e) for e in res] == [kinds.get(j, type(None)) for j in range(24)]
    mixed = [packed[j] if j % 2 else (base[j][0], packed[j][1]) for j in range(24)]
    mixed[12] = packed[12]
    res = verifier.verify_each(pvk, mixed)
    assert [type(e) for e in res] == [kinds.get(j, type(None)) for j in range(24)]
    assert _batch(mixed).find_invalid(random.Random(8), pvk) == [3, 9, 12]
    assert _batch(packed).find_invalid(random.Random(8), pvk) == [3, 9, 12]
    # a wrong input count: before any work
    wrong = list(base[:4])
    wrong[2] = (wrong[2][0], [])
    with pytest.raises(InvalidVerifyingKey):
        verifier.verify_each(pvk, wrong)
    with pytest.raises(InvalidVerifyingKey):
        _batch(wrong).find_invalid(random.Random(1), pvk)


# ---- 7. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(mimc, pool):  # noqa: F811
    pvk = mimc["pvk"]
    lib = _lib()
    items = pool["items"][:4]
    pr = b"".join(_proof_bytes(p) for p, _ in items)
    blob = b"".join(p.write() for p, _ in items)
    ins = b"".join(_raw(i[0]) for _, i in items)
    v = (ctypes.c_int32 * 4)()
    st = (ctypes.c_uint32 * 4)()
    # the key's input count first: even with every other argument wrong
    for n_in in (0, 2):
        assert lib.bh_groth16_verify_each(pvk._h, pr, 4, ins, n_in, 0, v, None) == INVALID_KEY
        assert lib.bh_groth16_verify_each(pvk._h, None, 4, None, n_in, 5, None, None) == INVALID_KEY
        assert lib.bh_groth16_verify_each_compressed(pvk._h, blob, 4, ins, n_in, 0, v, st, None) == INVALID_KEY
        assert lib.bh_groth16_verify_each_compressed(pvk._h, None, 4, None, n_in, 5, None, None, None) == INVALID_KEY
        assert lib.bh_groth16_verify_each(pvk._h, None, 0, None, n_in, 0, None, None) == INVALID_KEY
    assert lib.bh_groth16_verify_each(pvk._h, None, 4, ins, 1, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(pvk._h, pr, 4, None, 1, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(pvk._h, pr, 4, ins, 1, 0, None, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(None, pr, 4, ins, 1, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(pvk._h, pr, 4, ins, 1, 2, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(pvk._h, pr, 4, ins, 1, -1, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_compressed(pvk._h, None, 4, ins, 1, 0, v, st, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_compressed(pvk._h, blob, 4, None, 1, 0, v, st, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_compressed(pvk._h, blob, 4, ins, 1, 0, None, st, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_compressed(pvk._h, blob, 4, ins, 1, 7, v, st, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each(pvk._h, pr, 4, ins, 1, 0, v, None) == OK and list(v) == [OK] * 4
    assert lib.bh_groth16_verify_each_compressed(pvk._h, blob, 4, ins, 1, 0, v, st, None) == OK and list(v) == [OK] * 4


# ---- 8. four threads beside a 2^20-constraint proof ------------------------------------------------------------------------
def test_threads_beside_a_proof(worker, mimc, pool):  # noqa: F811
    """Run once.  A queue abort here is a finding about scratch or workspace (tools/kernel_resources.py pairing.hip)."""
    from bellman_amd import groth16 as pg

    pvk = mimc["pvk"]
    rounds = (1 << 20) - 3
    seed, x0, r, s = 2020, 987654321, 0xABCDEF0123, 0x123456789AB
    pp, _, _ = _chain_setup(worker, rounds, seed)
    alone = pg.create_proof_demo(pp, 1, rounds, seed, [x0], None, r, s)
    results = [None] * 4

    def run(k):
        rnd = random.Random(100 + k)
        items = list(pool["items"][k * 3000:(k + 1) * 3000])
        bad = sorted(rnd.sample(range(len(items)), 5 + k))
        for j in bad:
            items[j] = _wrong_input(items[j])
        rc, got, n_bad = _each(pvk, items)
        results[k] = rc == OK and [j for j, v in enumerate(got) if v] == bad and n_bad == len(bad) and \
            all(got[j] == INVALID_PROOF for j in bad)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    beside = pg.create_proof_demo(pp, 1, rounds, seed, [x0], None, r, s)
    for t in threads:
        t.join()
    assert results == [True] * 4
    assert (beside.a == alone.a).all() and (beside.b == alone.b).all() and (beside.c == alone.c).all()


# ---- 9. the shared-squaring form of the Miller stage (the benchmark's comparison) gives the same verdicts -------------------
def _shared_form_child():
    """runs in a process of its own (the switch is read once per process): 300 proofs, nine of them spoiled, judged by the
    three-pair shared-squaring loop; every spoiled proof and nine others against bh_groth16_verify"""
    os.environ["BELLMAN_HIP_VERIFY_EACH_SHARED"] = "1"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bellman_amd
    import bench_verify as bv
    from bellman_amd import verifier

    lib = _lib()
    w = bellman_amd.Worker(0)
    params, proofs, images = bv.fixture(w)
    pvk = verifier.prepare_verifying_key(params)
    n = 300
    recs, ins = bv.rerandomised(w, proofs, images, n)
    recs = recs.copy()
    want = [OK] * n
    for j in (0, 63, 64, 150, 299):
        ins[j] = (ins[j] + 1) % Q
        want[j] = INVALID_PROOF
    recs[7, 0] ^= np.uint64(1)          # A off its curve
    recs[70, 12] ^= np.uint64(1)        # B
    want[7] = want[70] = INVALID_POINT
    recs[200, :12] = 0                  # A the identity
    recs[201, 12:36] = 0                # B the identity
    want[200] = want[201] = INVALID_PROOF
    inputs = b"".join(_raw(v) for v in ins)
    verdicts = (ctypes.c_int32 * n)()
    n_bad = ctypes.c_size_t(0)
    p = recs.ctypes.data_as(ctypes.c_void_p)
    assert lib.bh_groth16_verify_each(pvk._h, p, n, inputs, 1, 0, verdicts, ctypes.byref(n_bad)) == OK
    assert list(verdicts) == want and n_bad.value == 9
    for j in [j for j in range(n) if want[j]] + list(range(20, 29)):
        assert lib.bh_groth16_verify(pvk._h, recs[j].ctypes.data_as(ctypes.c_void_p), _raw(ins[j]), 1, 0) == want[j], j
    pvk.release()
    w.close()
    print("shared form ok")


def test_shared_squaring_form_gives_the_same_verdicts():
    import subprocess

    env = dict(os.environ)
    env.pop("BELLMAN_HIP_VERIFY_EACH_SHARED", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shared-form-child"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "shared form ok"


if __name__ == "__main__":
    if sys.argv[1:] == ["--shared-form-child"]:
        _shared_form_child()
