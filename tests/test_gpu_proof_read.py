"""Compressed points and proofs on the device (bellman_amd/csrc/point_read.hip): Bases.read_compressed against the integer
model of tests/compressed_model.py for every rule of the encoding, round trips at scale cross-checked with the
uncompressed reader's [q] P kernel, Proof::read with the sequential reader's error precedence, and batch verification
straight from the bytes Proof::write emits (bh_groth16_batch_verify_compressed)."""

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
from tests import circuits, pointgen  # noqa: E402
from tests import compressed_model as cm  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401
from tests.test_gpu_verifier import _batch, _rerandomised, mimc  # noqa: E402,F401

pytestmark = pytest.mark.gpu
P, Q = bls.P, bls.Q


def _comp(group, pt):
    return bls.g1_compress(pt) if group == 1 else bls.g2_compress(pt)


def _records(group, pts):
    return cref.g1_from_py(pts) if group == 1 else cref.g2_from_py(pts)


def _torsion(group, seed):
    """a point of the curve whose order divides the cofactor"""
    curve = bls.G1 if group == 1 else bls.G2
    gen = pointgen.g1_on_curve_not_in_subgroup if group == 1 else pointgen.g2_on_curve_not_in_subgroup
    t = curve.mul(gen(seed), Q)
    assert t is not None and curve.on_curve(t)
    return t


def _non_residue_x(group):
    """an x < p for which x^3 + b is not a square"""
    x = 1
    while True:
        if group == 1:
            if pointgen._fp_sqrt((x ** 3 + 4) % P) is None:
                return x.to_bytes(48, "big")
        else:
            xx = (x, 1)
            if pointgen._fp2_sqrt(bls.fp2_add(bls.fp2_mul(bls.fp2_mul(xx, xx), xx), bls.G2_B)) is None:
                return xx[1].to_bytes(48, "big") + xx[0].to_bytes(48, "big")
        x += 1


def _read(worker, group, blob, checked, forbid):
    """(kind, index) or ("ok", records)"""
    import bellman_amd

    try:
        b = bellman_amd.Bases.read_compressed(worker, group, blob, checked=checked, forbid_identity=forbid)
    except bellman_amd.InvalidPoint as e:
        return cm.INVALID, e.index
    except bellman_amd.PointAtInfinity as e:
        return cm.INFINITY, e.index
    return "ok", b.download()


# ---- 1. the rules ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_read_compressed_rules_match_model(worker, group):
    curve = bls.G1 if group == 1 else bls.G2
    enc = 48 if group == 1 else 96
    good = [curve.mul(curve.gen, k) for k in (2, 3, 5, 7, 11, 13)]
    g = _comp(group, good[1])
    tors = pointgen.g1_on_curve_not_in_subgroup(9) if group == 1 else pointgen.g2_on_curve_not_in_subgroup(9)
    pure = _torsion(group, 21)
    nonres = bytearray(_non_residue_x(group))
    nonres[0] |= 0x80
    xp = bytearray(P.to_bytes(48, "big") + g[48:])
    xp[0] |= 0x80
    xp3 = bytearray((P + 3).to_bytes(48, "big") + g[48:])
    xp3[0] |= 0x80
    mutations = {
        "compressed flag clear": bytes([g[0] & 0x7F]) + g[1:],
        "x = p": bytes(xp),
        "x = p + small": bytes(xp3),
        "last coordinate = p": g[:-48] + (P.to_bytes(48, "big") if group == 2 else bytes(xp)[-48:]),
        "infinity + sort": bytes([0xE0]) + bytes(enc - 1),
        "infinity + a stray bit": bytes([0xC0]) + bytes(enc - 2) + b"\x01",
        "infinity + coordinates": bytes([g[0] | 0x40]) + g[1:],
        "non-residue x": bytes(nonres),
        "wrong sort flag": bytes([g[0] ^ 0x20]) + g[1:],          # the other root: -P, not an error
        "torsion point": _comp(group, tors),
        "pure cofactor torsion": _comp(group, pure),
        "torsion + subgroup sum": _comp(group, curve.add(pure, good[4])),
        "identity": _comp(group, None),
        "valid": g,
    }
    ok = [_comp(group, p) for p in good]
    seen = set()
    for name, bad in mutations.items():
        for pos in (0, 3, 5):
            blobs = list(ok)
            blobs[pos] = bad
            for checked in (False, True):
                for forbid in (False, True):
                    want = cm.read_points(group, b"".join(blobs), checked, forbid)
                    got = _read(worker, group, b"".join(blobs), checked, forbid)
                    seen.add(want[0])
                    if want[0] == "ok":
                        assert got[0] == "ok", (name, pos, checked, forbid, got)
                        assert (got[1] == _records(group, want[1])).all(), (name, pos, checked, forbid)
                    else:
                        assert got == want, (name, pos, checked, forbid)
    assert seen == {"ok", cm.INVALID, cm.INFINITY}
    assert cm.read_points(group, mutations["wrong sort flag"])[1] == [curve.neg(good[1])]
    assert cm.read_points(group, mutations["torsion point"], checked=False)[0] == "ok"
    # two bad points: the first in stream order is the one reported
    blobs = list(ok)
    blobs[4] = mutations["non-residue x"]
    blobs[2] = mutations["identity"]
    assert _read(worker, group, b"".join(blobs), True, True) == (cm.INFINITY, 2)
    assert _read(worker, group, b"".join(blobs), True, False) == (cm.INVALID, 4)
    assert _read(worker, group, b"", True, True)[1].shape[0] == 0


# ---- 2. round trip at scale -----------------------------------------------------------------------------------------
def _compress_from_uncompressed(group, raw, n):
    """the compressed encoding from the uncompressed one (x | y big-endian): x with the flags, the sort flag from y"""
    rec = 96 if group == 1 else 192
    out = bytearray()
    for i in range(n):
        r = raw[i * rec:(i + 1) * rec]
        x, y = r[:rec // 2], r[rec // 2:]
        y1 = int.from_bytes(y[:48], "big")
        largest = y1 > (P - 1) // 2 if (group == 1 or y1) else int.from_bytes(y[48:], "big") > (P - 1) // 2
        out += bytes([x[0] | 0x80 | (0x20 if largest else 0)]) + x[1:]
    return bytes(out)


@pytest.mark.parametrize("group,log_n", [(1, 14), (2, 12)])
def test_round_trip_at_scale_and_cross_check(worker, group, log_n):
    import bellman_amd

    n = 1 << log_n
    arr = cref.gen_bases(group, n, a=7, b=3)
    pts = (cref.g1_to_py if group == 1 else cref.g2_to_py)(arr)
    enc = bls.g1_uncompressed if group == 1 else bls.g2_uncompressed
    raw = b"".join(enc(p) for p in pts)
    blob = _compress_from_uncompressed(group, raw, n)
    for i in (0, 1, n // 2, n - 1):   # the shortcut above against the writer of oracle/pyref
        size = 48 if group == 1 else 96
        assert blob[i * size:(i + 1) * size] == _comp(group, pts[i])
    got = bellman_amd.Bases.read_compressed(worker, group, blob, checked=True).download()
    assert (got == arr).all()
    old = bellman_amd.Bases.read_uncompressed(worker, group, raw, checked=True).download()
    assert (old == got).all()
    assert (bellman_amd.Bases.read_compressed(worker, group, blob, checked=False).download() == arr).all()
    # one planted torsion point: both readers find it at its index
    where = n - 1234
    curve = bls.G1 if group == 1 else bls.G2
    t = curve.add(_torsion(group, 33), pts[5])
    size = 48 if group == 1 else 96
    rec = 2 * size
    blob2 = blob[:where * size] + _comp(group, t) + blob[(where + 1) * size:]
    raw2 = raw[:where * rec] + enc(t) + raw[(where + 1) * rec:]
    with pytest.raises(bellman_amd.InvalidPoint) as e:
        bellman_amd.Bases.read_compressed(worker, group, blob2, checked=True)
    assert e.value.index == where
    with pytest.raises(bellman_amd.InvalidPoint) as e:
        bellman_amd.Bases.read_uncompressed(worker, group, raw2, checked=True)
    assert e.value.index == where
    unchecked = bellman_amd.Bases.read_compressed(worker, group, blob2, checked=False).download()
    assert (unchecked[where] == _records(group, [t])[0]).all()


# ---- 3. Proof::read -------------------------------------------------------------------------------------------------
def _same_proof(a, b):
    return (a.a == b.a).all() and (a.b == b.b).all() and (a.c == b.c).all()


def _set(data, k, elem, enc):
    """proof k of the concatenated proofs with element a / b / c replaced"""
    lo = {"a": 0, "b": 48, "c": 144}[elem]
    return data[:192 * k + lo] + enc + data[192 * k + lo + len(enc):]


def test_proof_read_round_trip_and_precedence(worker, mimc):
    import bellman_amd
    from bellman_amd import groth16 as pg

    proofs = mimc["proofs"]
    for pr in proofs:
        data = pr.write()
        assert cm.read_proof(data)[0] == "ok"
        assert _same_proof(pg.Proof.read(worker, data), pr)
        assert pg.Proof.read(worker, data).write() == data
    with pytest.raises(bellman_amd.UnexpectedEof):
        pg.Proof.read(worker, proofs[0].write()[:191])
    assert pg.read_proofs(worker, b"") == []
    eight = [proofs[k % 4] for k in range(8)]
    data = b"".join(p.write() for p in eight)
    back = pg.read_proofs(worker, data)
    assert len(back) == 8 and all(_same_proof(x, y) for x, y in zip(back, eight))

    inf1, inf2 = bls.g1_compress(None), bls.g2_compress(None)
    bad1 = bls.g1_compress(pointgen.g1_on_curve_not_in_subgroup(3))
    bad2 = bls.g2_compress(pointgen.g2_on_curve_not_in_subgroup(3))

    def outcome(blob):
        try:
            pg.read_proofs(worker, blob)
        except bellman_amd.InvalidPoint as e:
            return cm.INVALID, e.index
        except bellman_amd.PointAtInfinity as e:
            return cm.INFINITY, e.index
        return "ok", None

    def model(blob):
        for k in range(len(blob) // 192):
            kind, _ = cm.read_proof(blob[192 * k:192 * k + 192])
            if kind != "ok":
                return kind, k
        return "ok", None

    cases = {
        "bad a, bad c": _set(_set(data, 2, "a", bad1), 2, "c", inf1),                 # a is reported: invalid
        "identity a, invalid b": _set(_set(data, 1, "a", inf1), 1, "b", bad2),        # a is reported: infinity
        "invalid b in 5, identity a in 3": _set(_set(data, 5, "b", bad2), 3, "a", inf1),   # proof 3 is reported
        "identity c": _set(data, 6, "c", inf1),
        "identity b": _set(data, 0, "b", inf2),
        "valid a, invalid c": _set(data, 7, "c", bad1),
    }
    want = {"bad a, bad c": (cm.INVALID, 2), "identity a, invalid b": (cm.INFINITY, 1),
            "invalid b in 5, identity a in 3": (cm.INFINITY, 3), "identity c": (cm.INFINITY, 6), "identity b": (cm.INFINITY, 0),
            "valid a, invalid c": (cm.INVALID, 7)}
    for name, blob in cases.items():
        assert model(blob) == want[name], name
        assert outcome(blob) == want[name], name

    # the status array marks EVERY bad proof of a batch with several
    blob = _set(_set(_set(_set(data, 1, "a", inf1), 1, "b", bad2), 4, "c", bad1), 6, "b", inf2)
    got, status = pg.read_proofs(worker, blob, return_status=True)
    assert [i for i in range(8) if status[i]] == [1, 4, 6]
    assert [g is None for g in got] == [s != 0 for s in status]
    assert all(_same_proof(got[i], eight[i]) for i in (0, 2, 3, 5, 7))
    assert status[1] & 0xFF == 0x10 and (status[1] >> 8) & 0xFF == 0x40      # a: identity, b: outside the subgroup
    assert status[4] == 0x40 << 16 and status[6] == 0x10 << 8
    assert outcome(blob) == (cm.INFINITY, 1)


# ---- 4. batch verification from bytes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_bytes(worker, mimc):
    """16384 + 1000 valid proofs as Proof::write emits them, with the affine proofs they came from"""
    items = _rerandomised(worker, mimc, 16384 + 1000, 99)
    return items, [(p.write(), ins) for p, ins in items]


def _a_plus_torsion(item):
    """the written proof with A replaced by A + T, T of order 3: still on the curve, outside the subgroup"""
    pr, _ = item
    a = cref.g1_to_py(pr.a.reshape(1, 12))[0]
    assert bls.G1.mul((0, 2), 3) is None
    t = bls.G1.add(a, (0, 2))
    assert bls.G1.on_curve(t) and bls.G1.mul(t, Q) is not None
    return t


def test_batch_verify_from_bytes(worker, mimc, many_bytes):
    import bellman_amd

    pvk = mimc["pvk"]
    affine, packed = many_bytes
    rnd = random.Random(15)
    for n in (1, 7, 1024, 16384, 16384 + 1000):
        _batch(packed[:n]).verify(rnd, pvk)
        _batch(affine[:n]).verify(rnd, pvk)               # the same verdict from the affine call
    _batch(affine[:3] + packed[3:9]).verify(rnd, pvk)     # a mixed batch reads its byte items first
    bellman_amd.verify_proof(pvk, packed[0][0], packed[0][1])
    # a corrupted public input
    for n, pos in ((7, 3), (16384 + 1000, 16384 + 500)):
        bad = list(packed[:n])
        bad[pos] = (bad[pos][0], [(bad[pos][1][0] + 1) % Q])
        with pytest.raises(bellman_amd.InvalidProof):
            _batch(bad).verify(rnd, pvk)
        aff = list(affine[:n])
        aff[pos] = (aff[pos][0], bad[pos][1])
        with pytest.raises(bellman_amd.InvalidProof):
            _batch(aff).verify(rnd, pvk)
    # A + T: the affine call's on-curve test passes it, the reader does not - in the first and in the second chunk
    for pos in (100, 16384 + 77):
        t = _a_plus_torsion(affine[pos])
        bad = list(packed)
        bad[pos] = (bls.g1_compress(t) + packed[pos][0][48:], packed[pos][1])
        with pytest.raises(bellman_amd.InvalidPoint) as e:
            _batch(bad).verify(rnd, pvk)
        assert e.value.index == pos
        # ... and still the read error with an additional wrong public input earlier in the batch
        bad[5] = (bad[5][0], [(bad[5][1][0] + 1) % Q])
        with pytest.raises(bellman_amd.InvalidPoint) as e:
            _batch(bad).verify(rnd, pvk)
        assert e.value.index == pos
        # the affine entry point makes only the on-curve test: the same point is no InvalidPoint there (what the pairing
        # of a point outside G1 gives is not specified: accepted or InvalidProof)
        from bellman_amd import groth16 as pg

        rec = affine[pos][0]
        tampered = pg.Proof(np.concatenate([cref.g1_from_py([t])[0], rec.b, rec.c]).astype(np.uint64))
        try:
            _batch([(tampered, affine[pos][1])]).verify(rnd, pvk)
        except bellman_amd.InvalidProof:
            pass
    with pytest.raises(bellman_amd.InvalidPoint):
        bellman_amd.verify_proof(pvk, bls.g1_compress(_a_plus_torsion(affine[0])) + packed[0][0][48:], packed[0][1])


def test_batch_from_bytes_argument_errors(mimc, many_bytes):
    from bellman_amd import InvalidVerifyingKey, _lib
    from bellman_amd.verifier import _fr_bytes

    pvk = mimc["pvk"]
    _, packed = many_bytes
    items = list(packed[:8])
    items[5] = (items[5][0], [])
    with pytest.raises(InvalidVerifyingKey):
        _batch(items).verify(random.Random(1), pvk)
    lib = _lib.load()
    pr = packed[0][0] + packed[1][0]
    ins = _fr_bytes([packed[0][1][0], packed[1][1][0]])
    bad = ctypes.c_size_t(0)
    assert lib.bh_groth16_batch_verify_compressed(pvk._h, pr, 2, ins, 1, 0, _fr_bytes([3, 0]), ctypes.byref(bad)) == -2
    assert lib.bh_groth16_batch_verify_compressed(pvk._h, pr, 2, ins, 1, 0, _fr_bytes([3, 5]), ctypes.byref(bad)) == 0
    assert lib.bh_groth16_batch_verify_compressed(pvk._h, pr, 2, ins, 1, 0, _fr_bytes([3, 5]), None) == 0
    assert lib.bh_groth16_batch_verify_compressed(pvk._h, None, 0, None, 1, 0, None, None) == 0


# ---- 5. concurrency ---------------------------------------------------------------------------------------------------
def test_batch_from_bytes_threads_beside_a_proof(worker, mimc, many_bytes):
    from bellman_amd import InvalidProof, verify_proof
    from bellman_amd import groth16 as pg

    pvk = mimc["pvk"]
    _, packed = many_bytes
    results = [None] * 4

    def run(k):
        rnd = random.Random(100 + k)
        items = list(packed[k * 200:(k + 1) * 200])
        want_ok = k % 2 == 0
        if not want_ok:
            pr, ins = items[7]
            items[7] = (pr, [(ins[0] + 1) % Q])
        try:
            _batch(items).verify(rnd, pvk)
            results[k] = want_ok
        except InvalidProof:
            results[k] = not want_ok

    rnd = random.Random(78)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    xl, xr = rnd.randrange(Q), rnd.randrange(Q)
    cons = mimc["cons"]
    proof = pg.create_random_proof(circuits.mimc_circuit(xl, xr, cons), mimc["params"], rng=rnd)
    for t in threads:
        t.join()
    assert results == [True] * 4
    verify_proof(pvk, proof.write(), [circuits.mimc_hash(xl, xr, cons)])
