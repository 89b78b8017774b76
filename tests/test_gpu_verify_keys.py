"""Proofs of several verifying keys in one call (bh_pvk_set, bh_groth16_verify_each_keys / _compressed,
bh_groth16_batch_verify_keys / _compressed; bellman_amd.verifier KeySet, verify_each_keys, MultiVerifier).

The contracts under test:
  verdicts[j] is the code bh_groth16_verify(pvks[key_of[j]], proof_j, inputs_j) returns for that proof alone (after
  bh_proofs_read, for bytes), whatever the interleaving of the keys;
  the batch check returns BH_OK exactly when prod_j E_j^{z_j} = 1 over all keys - one product, one final exponentiation
  (tests/models/verify_keys_model.py; pinned by tests/test_keyset_cpu.py).
All proof material comes from tests/models/pairing_stage_model.ScalarKey: keys with different tags have unrelated elements,
so a proof judged under the wrong key, or with another key's input offset, comes out INVALID_PROOF.  No tolerance anywhere:
integer work."""

import ctypes
import random
import threading

import numpy as np
import pytest

from oracle.pyref import bls12_381 as bls
from tests import compressed_model as cm
from tests import group_model as gm
from tests.models import pairing_stage_model as psm
from tests.models import verify_keys_model as vkm

pytestmark = pytest.mark.gpu
Q = psm.Q
OK, INVALID_POINT, AT_INFINITY, INVALID_PROOF, INVALID_KEY, INVALID_ARG = 0, 6, 7, 9, 8, -2
CHUNK = 16384
SENTINEL = -99


# -------------------------------------------------------------------------------------------------------------- material
class Row:
    """one proof of a call: the key's position in the set, the affine record, the inputs (integers, as given)"""

    def __init__(self, key, points, inputs):
        self.key, self.points, self.inputs = key, points, list(inputs)
        self.rec = psm.proof_rec(*points)

    def ident(self, fmt):
        return (self.key, self.rec, tuple(self.inputs), fmt)

    def with_key(self, key):
        return Row(key, self.points, self.inputs)


def g1_arr(pt):
    return np.frombuffer(psm.g1_rec(pt), dtype=np.uint64)


def g2_arr(pt):
    return np.frombuffer(psm.g2_rec(pt), dtype=np.uint64)


def make_pvk(worker, key):
    from bellman_amd import verifier

    return verifier.PreparedVerifyingKey.from_elements(worker, g1_arr(key.alpha), g2_arr(key.beta), g2_arr(key.gamma),
                                                       g2_arr(key.delta), np.stack([g1_arr(pt) for pt in key.ic]))


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def lib():
    from bellman_amd import _lib

    return _lib.load()


class Material:
    """four keys with 0, 1, 5 and 16 inputs, eight valid proofs of each (the first three statements of a key hold the edge
    scalars 0, 1, q - 1), their set, and the single-proof reference, computed once per distinct (key, proof, inputs, format)"""

    N_INPUTS = (0, 1, 5, 16)

    def __init__(self, worker, lib):
        from bellman_amd import verifier

        self.worker, self.lib = worker, lib
        self.keys = [psm.ScalarKey(n, "verify keys %d" % n) for n in self.N_INPUTS]
        self.pvks = [make_pvk(worker, k) for k in self.keys]
        self.set = verifier.KeySet(self.pvks)
        rnd = psm.rng("verify keys rows")
        edge = [0, 1, Q - 1]
        self.valid = []          # per key: rows
        for k, key in enumerate(self.keys):
            rows = []
            for t in range(8):
                ins = [edge[(t + i) % 3] if t < 3 else rnd.randrange(Q) for i in range(len(key.c) - 1)]
                rows.append(Row(k, key.proof(ins), ins))
            self.valid.append(rows)
        self._single = {}

    def single(self, row, fmt=psm.CANONICAL):
        """bh_groth16_verify of the row alone under its own key"""
        ident = row.ident(fmt)
        if ident not in self._single:
            ins = psm.fr_bytes(psm.scalar_raw(v, fmt) for v in row.inputs)
            self._single[ident] = self.lib.bh_groth16_verify(self.pvks[row.key]._h, row.rec, ins or None, len(row.inputs), fmt)
        return self._single[ident]

    def release(self):
        self.set.release()
        for p in self.pvks:
            p.release()


@pytest.fixture(scope="module")
def mat(worker, lib):
    m = Material(worker, lib)
    yield m
    m.release()


def each_keys(lib, keyset, rows, fmt=psm.CANONICAL, key_of=None, n_inputs_total=None):
    """bh_groth16_verify_each_keys -> (rc, verdicts, n_bad); verdicts and n_bad start as sentinels"""
    n = len(rows)
    ins = psm.fr_bytes(psm.scalar_raw(v, fmt) for r in rows for v in r.inputs)
    ko = (ctypes.c_uint32 * max(n, 1))(*(key_of if key_of is not None else [r.key for r in rows]))
    verdicts = (ctypes.c_int32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    n_bad = ctypes.c_size_t(12345)
    total = len(ins) // 32 if n_inputs_total is None else n_inputs_total
    rc = lib.bh_groth16_verify_each_keys(keyset._h, ko, b"".join(r.rec for r in rows) or None, n, ins or None, total, fmt, verdicts,
                                         ctypes.byref(n_bad))
    return rc, list(verdicts)[:n], n_bad.value


def batch_keys(lib, keyset, rows, zs, fmt=psm.CANONICAL):
    n = len(rows)
    ins = psm.fr_bytes(psm.scalar_raw(v, fmt) for r in rows for v in r.inputs)
    ko = (ctypes.c_uint32 * max(n, 1))(*[r.key for r in rows])
    z = psm.fr_bytes(zs if fmt == psm.CANONICAL else [psm.scalar_raw(v, fmt) for v in zs])
    return lib.bh_groth16_batch_verify_keys(keyset._h, ko, b"".join(r.rec for r in rows) or None, n, ins or None, len(ins) // 32,
                                            fmt, z or None)


def spoil(mat, row, kind, rnd):
    """one way of being bad each"""
    a, b, c = row.points
    g1, g2 = psm.g1_points(), psm.g2_points()
    if kind == "wrong input" and row.inputs:
        i = rnd.randrange(len(row.inputs))
        return Row(row.key, row.points, row.inputs[:i] + [(row.inputs[i] + 1) % Q] + row.inputs[i + 1:])
    if kind in ("wrong input", "wrong c"):     # (a key without inputs has no wrong input)
        return Row(row.key, (a, b, gm.add(1, c, gm.GEN[1])), row.inputs)
    if kind == "a off curve":
        return Row(row.key, (g1["off_curve"][0], b, c), row.inputs)
    if kind == "b off curve":
        return Row(row.key, (a, g2["off_curve"][0], c), row.inputs)
    if kind == "c off curve":
        return Row(row.key, (a, b, g1["off_curve"][1]), row.inputs)
    if kind == "a identity":
        return Row(row.key, (None, b, c), row.inputs)
    if kind == "b identity":
        return Row(row.key, (a, None, c), row.inputs)
    assert kind == "wrong key"                 # the right proof under another key's position, with that key's input count
    other = [k for k in (0, 1, 2) if k != row.key][rnd.randrange(2)]
    return Row(other, row.points, (row.inputs + [rnd.randrange(Q) for _ in range(16)])[:mat.N_INPUTS[other]])


KINDS = ("wrong input", "wrong c", "a off curve", "b off curve", "c off curve", "a identity", "b identity", "wrong key")


@pytest.fixture(scope="module")
def case1(mat):
    """131 rows sorted by key - 40 + 24 + 64 + 3: key boundaries inside a wave (row 40), at rows 63 / 64 and at row 128 -
    about a quarter of them bad; the row's own position in its key's run picks the proof"""
    rnd = random.Random(20250101)
    counts = (40, 24, 64, 3)
    picked = [(mat.valid[k][t % 8], False) for k, c in enumerate(counts) for t in range(c)]
    for n, j in enumerate(sorted(rnd.sample(range(len(picked)), 33))):
        picked[j] = (spoil(mat, picked[j][0], KINDS[n % len(KINDS)], rnd), True)
    # a row spoiled by its key's position has moved to another key: valid rows leave or join until the runs are 40 + 24 + 64 + 3 again
    rows = []
    for k, c in enumerate(counts):
        run = [(r, b) for r, b in picked if r.key == k]
        while len(run) > c:
            run.remove(next(e for e in reversed(run) if not e[1]))
        run += [(mat.valid[k][t % 8], False) for t in range(c - len(run))]
        rows += [r for r, _ in run]
    assert len(rows) == 131
    interleaved = []
    by_key = [[r for r in rows if r.key == k] for k in range(4)]
    for t in range(max(len(b) for b in by_key)):
        interleaved += [b[t] for b in by_key if t < len(b)]
    shuffled = list(rows)
    random.Random(7).shuffle(shuffled)
    return {"sorted": rows, "interleaved": interleaved, "shuffled": shuffled}


# ---- 1. the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [psm.CANONICAL, psm.MONT])
def test_verdicts_are_verify_proof_under_each_rows_own_key(lib, mat, case1, fmt):
    seen = set()
    for name, rows in case1.items():
        assert len(rows) == 131
        want = [mat.single(r, fmt) for r in rows]
        rc, got, n_bad = each_keys(lib, mat.set, rows, fmt)
        assert rc == OK, name
        assert got == want, name
        assert n_bad == sum(v != OK for v in want), name
        seen |= set(want)
    assert seen == {OK, INVALID_POINT, INVALID_PROOF}
    assert any(a.key != b.key for a, b in zip(case1["interleaved"], case1["interleaved"][1:]))
    keys_sorted = [r.key for r in case1["sorted"]]
    assert keys_sorted == sorted(keys_sorted) and keys_sorted[63] != keys_sorted[64]


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes(lib, mat, case1, n):
    rows = case1["interleaved"][:n]
    rc, got, n_bad = each_keys(lib, mat.set, rows)
    assert rc == OK and got == [mat.single(r) for r in rows] and n_bad == sum(v != OK for v in got)
    if n == 0:   # an empty call needs no pointers
        assert lib.bh_groth16_verify_each_keys(mat.set._h, None, None, 0, None, 0, 0, None, None) == OK
        assert lib.bh_groth16_verify_each_keys(mat.set._h, None, None, 0, None, 1, 0, None, None) == INVALID_KEY


def test_a_set_of_one_key_is_verify_each(lib, mat, case1):
    from bellman_amd import verifier

    rows = [r.with_key(0) for r in case1["sorted"] if r.key == 2] + [r.with_key(0) for r in mat.valid[2][:3]]
    assert len(rows) > 64
    one = verifier.KeySet([mat.pvks[2]])
    try:
        assert len(one) == 1 and lib.bh_groth16_pvk_set_len(one._h) == 1
        rc, got, n_bad = each_keys(lib, one, rows)
    finally:
        one.release()
    verdicts = (ctypes.c_int32 * len(rows))()
    ins = psm.fr_bytes(v for r in rows for v in r.inputs)
    assert lib.bh_groth16_verify_each(mat.pvks[2]._h, b"".join(r.rec for r in rows), len(rows), ins, 5, 0, verdicts, None) == OK
    assert rc == OK and got == list(verdicts) and n_bad == sum(v != OK for v in got)
    assert OK in got and INVALID_PROOF in got


@pytest.mark.parametrize("fmt", [psm.CANONICAL, psm.MONT])
@pytest.mark.parametrize("n", [1, 65])
def test_a_set_of_one_key_is_batch_verify(lib, mat, n, fmt):
    """the batch check over a set of one key returns what the one-key entry point returns, from records and from bytes: all
    rows valid, one invalid row, one unreadable row (the same bad_index too), a z equal to q"""
    from bellman_amd import verifier

    k = 2
    valid = [mat.valid[k][t % 8].with_key(0) for t in range(n)]
    rnd = random.Random(4242 + n)
    zs = [psm.scalar_raw(rnd.randrange(1, Q), fmt) for _ in range(n)]
    ko = (ctypes.c_uint32 * n)()
    one = verifier.KeySet([mat.pvks[k]])

    def both(rows, blobs, z_raw):
        """(set, one key) x (records -> code, bytes -> (code, bad_index)); blobs None: the rows as Proof::write writes them"""
        ins = psm.fr_bytes(psm.scalar_raw(v, fmt) for r in rows for v in r.inputs)
        recs, z = b"".join(r.rec for r in rows), psm.fr_bytes(z_raw)
        data = b"".join(blobs if blobs is not None else [compress(r.points) for r in rows])
        bad_set, bad_one = ctypes.c_size_t(777), ctypes.c_size_t(777)
        of_set = (lib.bh_groth16_batch_verify_keys(one._h, ko, recs, n, ins, len(ins) // 32, fmt, z),
                  (lib.bh_groth16_batch_verify_keys_compressed(one._h, ko, data, n, ins, len(ins) // 32, fmt, z, ctypes.byref(bad_set)),
                   bad_set.value))
        of_one = (lib.bh_groth16_batch_verify(mat.pvks[k]._h, recs, n, ins, mat.N_INPUTS[k], fmt, z),
                  (lib.bh_groth16_batch_verify_compressed(mat.pvks[k]._h, data, n, ins, mat.N_INPUTS[k], fmt, z, ctypes.byref(bad_one)),
                   bad_one.value))
        return of_set, of_one

    try:
        j = n // 2
        of_set, of_one = both(valid, None, zs)
        assert of_set == of_one == (OK, (OK, 777))
        invalid = list(valid)
        invalid[j] = spoil(mat, valid[j], "wrong c", rnd)
        of_set, of_one = both(invalid, None, zs)
        assert of_set == of_one == (INVALID_PROOF, (INVALID_PROOF, 777))
        blobs = [compress(r.points) for r in valid]
        blobs[j], code = unreadable(blobs[j], 1)
        of_set, of_one = both(valid, blobs, zs)                 # (the records are the valid rows: only the bytes are unreadable)
        assert of_set == of_one == (OK, (code, j)) and code == AT_INFINITY
        of_set, of_one = both(valid, None, zs[:j] + [Q] + zs[j + 1:])
        assert of_set == of_one == (INVALID_ARG, (INVALID_ARG, 777))
    finally:
        one.release()


def test_a_key_without_rows_the_same_key_twice_and_all_rows_on_the_last_key(lib, mat, case1):
    from bellman_amd import verifier

    rows = [r for r in case1["shuffled"] if r.key in (0, 2)]           # keys 1 and 3 of the set have no rows
    rc, got, _ = each_keys(lib, mat.set, rows)
    assert rc == OK and got == [mat.single(r) for r in rows]
    last = [r for r in case1["shuffled"] if r.key == 3] + mat.valid[3]  # every row on the last key
    rc, got, _ = each_keys(lib, mat.set, last)
    assert rc == OK and got == [mat.single(r) for r in last] and OK in got
    twice = verifier.KeySet([mat.pvks[1], mat.pvks[2], mat.pvks[1]])
    try:
        rows = [r for r in case1["interleaved"] if r.key in (1, 2)][:70]
        ones = [j for j, r in enumerate(rows) if r.key == 1]
        moved = [r.with_key(1 if r.key == 2 else (0, 2)[ones.index(j) % 2]) for j, r in enumerate(rows)]   # key 1 at both its positions
        assert {r.key for r in moved} == {0, 1, 2}
        rc, got, _ = each_keys(lib, twice, moved)
        assert rc == OK and got == [mat.single(r) for r in rows]
    finally:
        twice.release()


def test_edge_scalars_and_values_above_q(lib, mat):
    """inputs 0, 1, q - 1 (the first three statements of every key) and, in the canonical format, values >= q: whatever
    bh_groth16_verify makes of them"""
    rows = [mat.valid[k][t] for t in range(3) for k in (3, 1, 2)]
    rc, got, _ = each_keys(lib, mat.set, rows)
    assert rc == OK and got == [OK] * len(rows) == [mat.single(r) for r in rows]
    rc, got, _ = each_keys(lib, mat.set, rows, psm.MONT)
    assert rc == OK and got == [OK] * len(rows)
    big = []
    for j, r in enumerate(rows):
        ins = [v + Q if (i + j) % 2 == 0 and v + Q < 1 << 256 else v for i, v in enumerate(r.inputs)]
        if j % 4 == 1:
            ins[-1] = (1 << 256) - 1 - j        # another statement
        big.append(Row(r.key, r.points, ins))
    assert any(v >= Q for r in big for v in r.inputs)
    rc, got, _ = each_keys(lib, mat.set, big)
    want = [mat.single(r) for r in big]
    assert rc == OK and got == want and INVALID_PROOF in want


def test_an_identity_ic_entry_in_one_key_only(lib, worker, mat):
    from bellman_amd import verifier

    key = psm.ScalarKey(5, "verify keys identity ic")
    key.c[2], key.ic[2] = 0, None               # ic_2 the identity: the second input is free
    pvk = make_pvk(worker, key)
    keyset = verifier.KeySet([mat.pvks[2], pvk])
    try:
        rnd = psm.rng("identity ic rows")
        rows = []
        for t in range(6):
            ins = [rnd.randrange(Q) for _ in range(5)]
            proof = key.proof(ins)
            if t % 3 == 1:
                ins[1] = rnd.randrange(Q)       # free
            if t % 3 == 2:
                ins[2] = (ins[2] + 1) % Q       # not free
            rows.append(Row(1, proof, ins))
            rows.append(mat.valid[2][t].with_key(0))
            rows.append(mat.valid[2][t].with_key(1))    # the same statement under the key with the identity: wrong key
        want = [lib.bh_groth16_verify((mat.pvks[2], pvk)[r.key]._h, r.rec, psm.fr_bytes(r.inputs), 5, 0) for r in rows]
        assert want == [(INVALID_PROOF if j // 3 % 3 == 2 else OK) if j % 3 == 0 else OK if j % 3 == 1 else INVALID_PROOF
                        for j in range(len(rows))]
        rc, got, _ = each_keys(lib, keyset, rows)
        assert rc == OK and got == want
        rc = batch_keys(lib, keyset, [r for r, v in zip(rows, want) if v == OK], list(range(3, 3 + want.count(OK))))
        assert rc == OK
    finally:
        keyset.release()
        pvk.release()


# ---- 3. table widths differ inside one set ---------------------------------------------------------------------------------
def test_table_widths_differ_inside_one_set(lib, worker, mat):
    from bellman_amd import verifier

    start = worker.info()["table_bytes"]
    budget = worker.info()["table_budget"]
    pvks = [make_pvk(worker, mat.keys[3]), make_pvk(worker, mat.keys[3])]
    keyset = verifier.KeySet(pvks)
    rows = [r.with_key(j % 2) for j, r in enumerate(mat.valid[3] + mat.valid[3])]
    rows[5] = spoil(mat, rows[5], "wrong input", random.Random(5))
    rows[6] = spoil(mat, rows[6], "wrong c", random.Random(6))
    want = [mat.single(r.with_key(3)) for r in rows]
    try:
        before = worker.info()["table_bytes"]
        # room for the first key's 8-bit table and nothing more: the second key falls through 4 and 2 bits to the floor
        worker.set_limits(table_budget_bytes=before + psm.table_bytes(16, 8))
        rc, got, _ = each_keys(lib, keyset, rows)
        assert worker.info()["table_bytes"] - before == psm.table_bytes(16, 8) + psm.table_bytes(16, 1)
        assert rc == OK and got == want and want.count(INVALID_PROOF) == 2
        rc, got, _ = each_keys(lib, keyset, rows, psm.MONT)
        assert rc == OK and got == want
    finally:
        keyset.release()
        for p in pvks:
            p.release()
        worker.set_limits(table_budget_bytes=budget)
    info = worker.info()
    assert info["table_budget"] == budget and info["table_bytes"] == start


# ---- 4. 64 keys ----------------------------------------------------------------------------------------------------------------
def derived_keys(count):
    """`count` ScalarKeys with 0, 1, 2, 0, ... inputs, all elements different, made from one seed key by ADDITIONS: a
    ScalarKey costs 70 ms of Python multiplications, 64 of them more than the whole test may take.  The discrete logs of key
    k are the seed's plus k + 1 times a fixed random step, the points follow by one addition each; then one valid proof per
    key over shared A = [r] G1 and B = [s] G2: C = [c] G1 with c from E = 0 (tests/models/verify_keys_model.py)."""
    seed = psm.ScalarKey(2, "sixty-four seed")
    rnd = psm.rng("sixty-four steps")
    names = ("a", "b", "g", "d", "c0", "c1", "c2")
    logs = dict(zip(names, [seed.a, seed.b, seed.g, seed.d] + seed.c))
    pts = dict(zip(names, [seed.alpha, seed.beta, seed.gamma, seed.delta] + seed.ic))
    group = dict(zip(names, (1, 2, 2, 2, 1, 1, 1)))
    steps = {n: rnd.randrange(1, Q) for n in names}
    step_pts = {n: gm.mul(group[n], gm.GEN[group[n]], steps[n]) for n in names}
    r, s = rnd.randrange(1, Q), rnd.randrange(1, Q)
    a_pt, b_pt = gm.mul(1, gm.GEN[1], r), gm.mul(2, gm.GEN[2], s)
    keys, rows = [], []
    for k in range(count):
        logs = {n: (logs[n] + steps[n]) % Q for n in names}
        pts = {n: gm.add(group[n], pts[n], step_pts[n]) for n in names}
        key = object.__new__(psm.ScalarKey)
        key.a, key.b, key.g, key.d = (logs[n] for n in "abgd")
        key.alpha, key.beta, key.gamma, key.delta = (pts[n] for n in "abgd")
        key.c = [logs[n] for n in names[4:5 + k % 3]]
        key.ic = [pts[n] for n in names[4:5 + k % 3]]
        ins = [(k * 1000003 + i) % Q for i in range(k % 3)]
        acc = key.c[0] + sum(x * c for x, c in zip(ins, key.c[1:]))
        c = (r * s - key.a * key.b - acc * key.g) * pow(key.d, -1, Q) % Q
        assert vkm.exponent(key, (r, s, c), ins) == 0
        keys.append(key)
        rows.append(Row(k, (a_pt, b_pt, gm.mul(1, gm.GEN[1], c)), ins))
    return keys, rows


def test_sixty_four_keys(lib, worker):
    from bellman_amd import verifier

    keys, good_rows = derived_keys(64)
    assert len({k.delta for k in keys}) == 64 and len({k.ic[0] for k in keys}) == 64
    pvks = [make_pvk(worker, key) for key in keys]
    keyset = None
    try:
        keyset = verifier.KeySet(pvks)
        assert len(keyset) == 64 == lib.bh_groth16_pvk_set_len(keyset._h)
        rows = []
        for k, good in enumerate(good_rows):
            rows += [good, Row(k, vkm.shift_c(good.points, 1), good.inputs) if k % 3 == 0
                     else good.with_key(k + 3 if k + 3 < 64 else k - 3) if k % 3 == 1 else good]
        want = [lib.bh_groth16_verify(pvks[r.key]._h, r.rec, psm.fr_bytes(r.inputs) or None, len(r.inputs), 0) for r in rows]
        assert want == [OK if j % 2 == 0 or j // 2 % 3 == 2 else INVALID_PROOF for j in range(128)]
        rc, got, n_bad = each_keys(lib, keyset, rows)
        assert rc == OK and got == want and n_bad == want.count(INVALID_PROOF)
        passing = [r for r, v in zip(rows, want) if v == OK]
        assert batch_keys(lib, keyset, passing, list(range(1, len(passing) + 1))) == OK
        assert batch_keys(lib, keyset, rows, list(range(1, 129))) == INVALID_PROOF
        handles = (ctypes.c_void_p * 65)(*[p._h for p in pvks + pvks[:1]])
        h = ctypes.c_void_p()
        assert lib.bh_groth16_pvk_set_create(handles, 65, ctypes.byref(h)) == INVALID_ARG and not h.value
        assert lib.bh_groth16_pvk_set_create(handles, 0, ctypes.byref(h)) == INVALID_ARG
        handles[3] = None
        assert lib.bh_groth16_pvk_set_create(handles, 8, ctypes.byref(h)) == INVALID_ARG
    finally:
        if keyset is not None:
            keyset.release()
        for p in pvks:
            p.release()


def test_keys_of_two_contexts_are_refused(lib, mat):
    import bellman_amd

    other = bellman_amd.Worker(0)
    pvk = make_pvk(other, mat.keys[0])
    try:
        handles = (ctypes.c_void_p * 2)(mat.pvks[0]._h, pvk._h)
        h = ctypes.c_void_p()
        assert lib.bh_groth16_pvk_set_create(handles, 2, ctypes.byref(h)) == INVALID_ARG and not h.value
    finally:
        pvk.release()
        other.close()


# ---- 5. over one chunk -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_rows(mat):
    """16384 + 67 valid rows over keys 1, 2 and 3, repeating the distinct proofs, neighbours of different keys"""
    return [mat.valid[1 + j % 3][(j // 3) % 8] for j in range(CHUNK + 67)]


def test_over_one_chunk(lib, mat, long_rows):
    rows = list(long_rows)
    rnd = random.Random(55)
    bad = [0, 700, CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 66]
    for n, j in enumerate(bad):
        rows[j] = spoil(mat, rows[j], KINDS[n % len(KINDS)], rnd)
    want = [mat.single(r) for r in rows]
    assert [j for j, v in enumerate(want) if v != OK] == bad
    rc, got, n_bad = each_keys(lib, mat.set, rows)
    assert rc == OK and got == want and n_bad == len(bad)


# ---- 6. bytes ------------------------------------------------------------------------------------------------------------------
def compress(points):
    return bls.g1_compress(points[0]) + bls.g2_compress(points[1]) + bls.g1_compress(points[2])


def unreadable(data, how):
    """192 bytes that Proof::read refuses, by tests/compressed_model.py: (bytes, the reader's error code)"""
    data = bytearray(data)
    if how == 0:      # A: the compression flag clear
        data[0] &= 0x7F
    elif how == 1:    # B: a well-formed identity
        data[48:144] = bls.g2_compress(None)
    elif how == 2:    # C: x^3 + 4 is not a square
        x = 1
        while cm.from_compressed(1, bytes([0x80]) + x.to_bytes(48, "big")[1:])[0] == "ok":
            x += 1
        data[144:192] = bytes([0x80]) + x.to_bytes(48, "big")[1:]
    else:             # A: on the curve, outside the subgroup
        data[0:48] = bls.g1_compress(psm.g1_off_subgroup())
    kind, _ = cm.read_proof(bytes(data))
    assert kind in (cm.INVALID, cm.INFINITY)
    return bytes(data), INVALID_POINT if kind == cm.INVALID else AT_INFINITY


def each_keys_bytes(lib, keyset, items, key_of):
    n = len(items)
    ins = psm.fr_bytes(v for _, i in items for v in i)
    verdicts = (ctypes.c_int32 * n)(*([SENTINEL] * n))
    status = (ctypes.c_uint32 * n)(*([0xDEAD] * n))
    n_bad = ctypes.c_size_t(12345)
    rc = lib.bh_groth16_verify_each_keys_compressed(keyset._h, (ctypes.c_uint32 * n)(*key_of), b"".join(d for d, _ in items), n,
                                                    ins or None, len(ins) // 32, 0, verdicts, status, ctypes.byref(n_bad))
    return rc, list(verdicts), list(status), n_bad.value


@pytest.fixture(scope="module")
def packed(mat, case1):
    """70 rows of case 1 as bytes (rows with an off-curve or identity point are replaced by valid ones: they have no
    encoding), one unreadable row per key: (key_of, [(192 bytes, inputs)], {position: reader's code})"""
    rows = []
    for r in case1["interleaved"][:70]:
        ok = all(pt is not None for pt in r.points) and gm.on_curve(1, r.points[0]) and gm.on_curve(2, r.points[1]) and \
            gm.on_curve(1, r.points[2])
        rows.append(r if ok else mat.valid[r.key][0])
    rows[5] = Row(rows[5].key, vkm.shift_c(mat.valid[rows[5].key][1].points, 3), mat.valid[rows[5].key][1].inputs)
    items = [(compress(r.points), r.inputs) for r in rows]
    codes = {}
    for k in range(4):
        j = [j for j in range(6, 70) if rows[j].key == k][1]     # (the key's second row from row 6 on)
        data, code = unreadable(items[j][0], k)
        items[j] = (data, items[j][1])
        codes[j] = code
    return [r.key for r in rows], items, codes


def test_compressed_verdicts_and_status_words_are_those_of_each_key(lib, mat, packed):
    key_of, items, codes = packed
    rc, got, status, n_bad = each_keys_bytes(lib, mat.set, items, key_of)
    assert rc == OK
    for k in range(4):   # bh_groth16_verify_each_compressed, key by key
        where = [j for j in range(len(items)) if key_of[j] == k]
        n = len(where)
        verdicts = (ctypes.c_int32 * n)()
        words = (ctypes.c_uint32 * n)()
        ins = psm.fr_bytes(v for j in where for v in items[j][1])
        assert lib.bh_groth16_verify_each_compressed(mat.pvks[k]._h, b"".join(items[j][0] for j in where), n, ins or None,
                                                     mat.N_INPUTS[k], 0, verdicts, words, None) == OK
        assert [got[j] for j in where] == list(verdicts), k
        assert [status[j] for j in where] == list(words), k
    assert n_bad == sum(v != OK for v in got)
    for j, code in codes.items():
        assert got[j] == code and status[j] != 0
    assert {OK, INVALID_PROOF, INVALID_POINT, AT_INFINITY} <= set(got)
    assert all(status[j] == 0 for j in range(len(items)) if j not in codes)
    # status and n_bad are optional
    n = len(items)
    verdicts = (ctypes.c_int32 * n)()
    ins = psm.fr_bytes(v for _, i in items for v in i)
    assert lib.bh_groth16_verify_each_keys_compressed(mat.set._h, (ctypes.c_uint32 * n)(*key_of), b"".join(d for d, _ in items), n,
                                                      ins, len(ins) // 32, 0, verdicts, None, None) == OK
    assert list(verdicts) == got


# ---- 7. call-level errors ---------------------------------------------------------------------------------------------------
def test_call_level_errors_leave_the_verdicts_untouched(lib, mat, case1):
    rows = case1["interleaved"][:20]
    key_of = [r.key for r in rows]
    total = sum(len(r.inputs) for r in rows)
    for j in (0, 7, 19):
        rc, got, n_bad = each_keys(lib, mat.set, rows, key_of=key_of[:j] + [4] + key_of[j + 1:])
        assert rc == INVALID_ARG and got == [SENTINEL] * 20
    for off in (-1, 1):
        rc, got, _ = each_keys(lib, mat.set, rows, n_inputs_total=total + off)
        assert rc == INVALID_KEY and got == [SENTINEL] * 20
    # a row moved to a key with another input count: the sum no longer matches
    moved = list(key_of)
    moved[3] = (moved[3] + 1) % 4
    rc, got, _ = each_keys(lib, mat.set, rows, key_of=moved)
    assert rc == INVALID_KEY and got == [SENTINEL] * 20
    rc, got, _ = each_keys(lib, mat.set, rows, fmt=2)
    assert rc == INVALID_ARG and got == [SENTINEL] * 20
    ko = (ctypes.c_uint32 * 20)(*key_of)
    recs, ins = b"".join(r.rec for r in rows), psm.fr_bytes(v for r in rows for v in r.inputs)
    v = (ctypes.c_int32 * 20)()
    assert lib.bh_groth16_verify_each_keys(None, ko, recs, 20, ins, total, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_keys(mat.set._h, None, recs, 20, ins, total, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_keys(mat.set._h, ko, None, 20, ins, total, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_keys(mat.set._h, ko, recs, 20, None, total, 0, v, None) == INVALID_ARG
    assert lib.bh_groth16_verify_each_keys(mat.set._h, ko, recs, 20, ins, total, 0, None, None) == INVALID_ARG
    rc, got, _ = each_keys(lib, mat.set, rows)
    assert rc == OK and got == [mat.single(r) for r in rows]


# ---- 8. the batch: all valid, one bad -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def valid131(mat):
    counts = (40, 24, 64, 3)
    by_key = [[mat.valid[k][t % 8] for t in range(c)] for k, c in enumerate(counts)]
    rows = []
    for t in range(64):
        rows += [b[t] for b in by_key if t < len(b)]
    return rows


@pytest.mark.parametrize("fmt", [psm.CANONICAL, psm.MONT])
def test_batch_all_valid_and_any_one_row_bad(lib, mat, valid131, fmt):
    rnd = random.Random(88 + fmt)
    rows = valid131
    zs = [rnd.randrange(1, Q) for _ in rows]
    assert batch_keys(lib, mat.set, rows, zs, fmt) == OK
    for k in range(4):
        where = [j for j, r in enumerate(rows) if r.key == k]
        for j in (where[0], where[len(where) // 2], where[-1]):
            bad = list(rows)
            bad[j] = spoil(mat, rows[j], ("wrong input", "wrong c", "wrong key")[(j + k) % 3], rnd)
            assert batch_keys(lib, mat.set, bad, zs, fmt) == INVALID_PROOF, (k, j)


# ---- 9. the batch equals the exponent model, cancellation included ----------------------------------------------------------
def test_batch_is_one_product_under_one_final_exponentiation(lib, mat):
    k1, k2 = 1, 2
    rnd = random.Random(99)
    rows = [mat.valid[k1][0], mat.valid[k2][0], mat.valid[k1][1], mat.valid[k2][1], mat.valid[k1][2], mat.valid[k2][2], mat.valid[3][0]]
    zs = [rnd.randrange(1, Q) for _ in rows]
    i1, i2 = 2, 3                                   # the bad proof under each key
    t1 = rnd.randrange(1, Q)

    def with_shifts(t_1, t_2):
        out = list(rows)
        out[i1] = Row(k1, vkm.shift_c(rows[i1].points, t_1), rows[i1].inputs)
        out[i2] = Row(k2, vkm.shift_c(rows[i2].points, t_2), rows[i2].inputs)
        return out

    def per_key(batch, k):
        sub = [(r, z) for r, z in zip(batch, zs) if r.key == k]
        ins = psm.fr_bytes(v for r, _ in sub for v in r.inputs)
        return lib.bh_groth16_batch_verify(mat.pvks[k]._h, b"".join(r.rec for r, _ in sub), len(sub), ins, mat.N_INPUTS[k], 0,
                                           psm.fr_bytes(z for _, z in sub))

    assert batch_keys(lib, mat.set, rows, zs) == OK
    # random shifts: the exponent is -(z1 t1 d1 + z2 t2 d2) != 0
    t2 = rnd.randrange(1, Q)
    e = vkm.batch_exponent([(zs[i1], -t1 * mat.keys[k1].d), (zs[i2], -t2 * mat.keys[k2].d)])
    assert e != 0
    assert batch_keys(lib, mat.set, with_shifts(t1, t2), zs) == INVALID_PROOF
    # the shift that cancels across the keys: one product, so the call passes; every key alone fails
    t2 = vkm.cancelling_shift(mat.keys[k1], zs[i1], t1, mat.keys[k2], zs[i2])
    assert vkm.batch_exponent([(zs[i1], -t1 * mat.keys[k1].d), (zs[i2], -t2 * mat.keys[k2].d)]) == 0
    batch = with_shifts(t1, t2)
    assert batch_keys(lib, mat.set, batch, zs) == OK
    assert per_key(batch, k1) == INVALID_PROOF and per_key(batch, k2) == INVALID_PROOF and per_key(batch, 3) == OK
    rc, got, _ = each_keys(lib, mat.set, batch)
    assert rc == OK and got == [INVALID_PROOF if j in (i1, i2) else OK for j in range(len(rows))]
    # ... and with another z the same two proofs are caught
    zs[i2] = zs[i2] % (Q - 1) + 1
    assert batch_keys(lib, mat.set, batch, zs) == INVALID_PROOF


# ---- 10. the batch's call-level behaviour ---------------------------------------------------------------------------------------
def test_batch_call_level(lib, mat, valid131, long_rows):
    rows = valid131[:12]
    zs = list(range(5, 17))
    assert batch_keys(lib, mat.set, rows, zs) == OK
    for zero in (0, Q, 2 * Q):
        assert batch_keys(lib, mat.set, rows, zs[:7] + [zero] + zs[8:]) == INVALID_ARG
    off = list(rows)
    off[4] = spoil(mat, rows[4], "b off curve", None)
    off[5] = spoil(mat, rows[5], "wrong c", None)
    assert batch_keys(lib, mat.set, off, zs) == INVALID_POINT         # before INVALID_PROOF
    assert batch_keys(lib, mat.set, [], []) == OK
    assert lib.bh_groth16_batch_verify_keys(mat.set._h, None, None, 0, None, 0, 0, None) == OK
    ko = (ctypes.c_uint32 * 12)(*[r.key for r in rows])
    ins = psm.fr_bytes(v for r in rows for v in r.inputs)
    recs, z = b"".join(r.rec for r in rows), psm.fr_bytes(zs)
    assert lib.bh_groth16_batch_verify_keys(mat.set._h, ko, recs, 12, ins, len(ins) // 32 + 1, 0, z) == INVALID_KEY
    ko[2] = 4
    assert lib.bh_groth16_batch_verify_keys(mat.set._h, ko, recs, 12, ins, len(ins) // 32, 0, z) == INVALID_ARG
    # across a chunk
    rnd = random.Random(1010)
    zl = [rnd.randrange(1, Q) for _ in long_rows]
    assert batch_keys(lib, mat.set, long_rows, zl) == OK
    bad = list(long_rows)
    bad[-1] = spoil(mat, bad[-1], "wrong input", rnd)
    assert batch_keys(lib, mat.set, bad, zl) == INVALID_PROOF


def test_batch_compressed_reports_the_first_unreadable_row_in_the_callers_order(lib, mat, valid131):
    rows = valid131[:40]
    items = [compress(r.points) for r in rows]
    key_of = [r.key for r in rows]
    ko = (ctypes.c_uint32 * 40)(*key_of)
    ins = psm.fr_bytes(v for r in rows for v in r.inputs)
    z = psm.fr_bytes(range(3, 43))

    def run(blobs):
        bad = ctypes.c_size_t(777)
        rc = lib.bh_groth16_batch_verify_keys_compressed(mat.set._h, ko, b"".join(blobs), 40, ins, len(ins) // 32, 0, z,
                                                         ctypes.byref(bad))
        return rc, bad.value

    assert run(items) == (OK, 777)
    # the caller's first unreadable row (of key 3) stands behind a later one (of key 0) in the grouped order
    first = next(j for j in range(5, 40) if key_of[j] == 3)
    later = next(j for j in range(first + 1, 40) if key_of[j] == 0)
    blobs = list(items)
    blobs[first], code_first = unreadable(items[first], 1)
    blobs[later], code_later = unreadable(items[later], 0)
    assert code_first == AT_INFINITY and code_later == INVALID_POINT
    assert run(blobs) == (AT_INFINITY, first)
    blobs[first] = items[first]
    assert run(blobs) == (INVALID_POINT, later)
    # a read error wins over a bad proof
    blobs[2] = compress(vkm.shift_c(rows[2].points, 1))
    assert run(blobs) == (INVALID_POINT, later)
    blobs[later] = items[later]
    assert run(blobs)[0] == INVALID_PROOF


# ---- 11. the Python layer ---------------------------------------------------------------------------------------------------------
def as_proof(row):
    from bellman_amd import groth16 as pg

    return pg.Proof(np.frombuffer(row.rec, dtype=np.uint64).copy())


def test_python_layer(lib, mat, case1, valid131):
    import bellman_amd
    from bellman_amd import InvalidPoint, InvalidProof, InvalidVerifyingKey, PointAtInfinity, verifier

    assert bellman_amd.verify_each_keys is verifier.verify_each_keys
    rows = valid131[:30]
    rnd = random.Random(11)
    bad = [4, 17, 29]
    rows = [spoil(mat, r, "wrong input", rnd) if j in bad else r for j, r in enumerate(rows)]
    mv = verifier.MultiVerifier()
    for r in rows:
        mv.queue(r.key, (as_proof(r), r.inputs))
    assert mv.find_invalid(random.Random(1), mat.set) == bad
    with pytest.raises(InvalidProof):
        mv.verify(random.Random(2), mat.set)
    with pytest.raises(InvalidProof):
        mv.verify_multicore(mat.set)
    good = verifier.MultiVerifier()
    for r in valid131[:30]:
        good.queue(r.key, verifier.Item(compress(r.points), r.inputs))     # bytes only: the compressed entry point
    assert good.verify(random.Random(3), mat.set) is None and good.verify_multicore(mat.set) is None
    assert good.find_invalid(random.Random(4), mat.set) == [] and good.verify_each(mat.set) == [None] * 30
    assert verifier.MultiVerifier().find_invalid(random.Random(5), mat.set) == [] and verifier.verify_each_keys(mat.set, []) == []
    # mixed bytes / Proof items: None or the exception Item.verify_single raises under the item's own key
    sample = [r for r in case1["shuffled"][:24]]
    items = []
    for j, r in enumerate(sample):
        encodable = all(pt is not None for pt in r.points) and gm.on_curve(1, r.points[0]) and gm.on_curve(2, r.points[1]) and \
            gm.on_curve(1, r.points[2])
        items.append((r.key, compress(r.points) if encodable and j % 2 else as_proof(r), r.inputs))
    for j, how in ((1, 1), (3, 3)):       # two unreadable byte items, a wrong C and an off-curve A as Proof items
        good_row = mat.valid[items[j][0]][j]
        items[j] = (good_row.key, unreadable(compress(good_row.points), how)[0], good_row.inputs)
    for j, kind in ((5, "wrong c"), (7, "a off curve")):
        r = spoil(mat, mat.valid[items[j][0]][j], kind, None)
        items[j] = (r.key, as_proof(r), r.inputs)
    res = verifier.verify_each_keys(mat.set, items)
    kinds = set()
    for (k, proof, ins), e in zip(items, res):
        try:
            verifier.Item(proof, ins).verify_single(mat.pvks[k])
            assert e is None
        except (InvalidProof, InvalidPoint, PointAtInfinity) as err:
            assert type(e) is type(err)
        kinds.add(type(e))
    assert kinds == {type(None), InvalidProof, InvalidPoint, PointAtInfinity}
    mixed = verifier.MultiVerifier()
    for k, proof, ins in items:
        mixed.queue(k, (proof, ins))
    assert mixed.find_invalid(random.Random(6), mat.set) == [j for j, e in enumerate(res) if e is not None]
    # a wrong input count for the item's key: before any work
    wrong = [(r.key, as_proof(r), r.inputs) for r in valid131[:6]]
    wrong[2] = (wrong[2][0], wrong[2][1], wrong[2][2] + [1])
    with pytest.raises(InvalidVerifyingKey):
        verifier.verify_each_keys(mat.set, wrong)
    mw = verifier.MultiVerifier()
    for k, proof, ins in wrong:
        mw.queue(k, (proof, ins))
    for call in (lambda: mw.verify(random.Random(7), mat.set), lambda: mw.verify_multicore(mat.set), lambda: mw.verify_each(mat.set),
                 lambda: mw.find_invalid(random.Random(8), mat.set)):
        with pytest.raises(InvalidVerifyingKey):
            call()


# ---- 12. four threads share one set ---------------------------------------------------------------------------------------------
def test_four_threads_share_one_set(lib, mat, case1):
    names = ["sorted", "interleaved", "shuffled", "interleaved"]
    want = [[mat.single(r) for r in case1[name]] for name in names]
    results = [None] * 4

    def run(t):
        results[t] = each_keys(lib, mat.set, case1[names[t]], psm.MONT if t == 3 else psm.CANONICAL)

    want[3] = [mat.single(r, psm.MONT) for r in case1[names[3]]]
    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(4):
        assert results[t] == (OK, want[t], sum(v != OK for v in want[t])), t
