"""bh_groth16_assemble_many on the device (csrc/proof_finish.hip): k proofs from k sets of multiexp sums in one call, every
record held byte for byte against bh_groth16_assemble for its row - and against the host compilation of the same device
functions (bh_test_proof_finish_host) and the exponent arithmetic of tests/models/proof_finish_cases.py.  The rows mix
that module's corner table (identity elements, additions that meet their operand or its negative, scalars with a zero
split half) with random rows; the batch sizes sit on both sides of a 64-lane block for the one-lane-per-proof kernels
(63, 64, 65) and give the eight-lanes-per-proof kernel whole and ragged blocks (k = 1, 2, 130)."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bellman_amd import _lib  # noqa: E402
from bellman_amd.groth16 import fr_to_mont_array  # noqa: E402
from tests.models import proof_finish_cases as cases  # noqa: E402
from tests.test_gpu_groth16 import worker  # noqa: E402,F401

SENTINEL = 0xA5A5A5A5A5A5A5A5


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _params(worker, key=None):  # noqa: F811
    from bellman_amd import groth16 as pg

    rec = cases.key_records(key)
    q1, q2 = cases.point(1, 3).reshape(1, 12), cases.point(2, 3).reshape(1, 24)   # the queries are never read here
    return pg.Parameters(worker, rec["alpha_g1"], rec["beta_g1"], rec["beta_g2"], rec["delta_g1"], rec["delta_g2"], q1, q1, q1, q1, q2)


@pytest.fixture(scope="module")
def params(worker):  # noqa: F811
    return _params(worker)


@pytest.fixture(scope="module")
def table(params):
    """130 rows - every corner row, then random ones - with bh_groth16_assemble's record for each, computed once"""
    corner = cases.corner_rows()
    rows = [corner[n] for n in sorted(corner)]
    rows += cases.random_rows(130 - len(rows), 0xA55)
    lib = _lib.load()
    sums = np.ascontiguousarray(np.stack([cases.sums_record(row) for row in rows]))
    r, s = fr_to_mont_array([row["r"] for row in rows]), fr_to_mont_array([row["s"] for row in rows])
    want = np.zeros((len(rows), 48), dtype=np.uint64)
    for j in range(len(rows)):
        assert lib.bh_groth16_assemble(params._h, _p(sums[j]), _p(r[j]), _p(s[j]), _p(want[j])) == 0
    return rows, sums, r, s, want


def _pick(table, k):
    """k rows: corner rows and random rows interleaved, a different mix for every k"""
    rows, sums, r, s, want = table
    n = len(rows)
    idx = np.array([(7 * j + k) % n for j in range(k)] if k < n else list(range(n)))
    return idx, np.ascontiguousarray(sums[idx]), np.ascontiguousarray(r[idx]), np.ascontiguousarray(s[idx]), want[idx]


def test_the_reference_records_equal_the_exponent_arithmetic(table):
    rows, _, _, _, want = table
    for j in (0, 5, 11, len(rows) - 1):
        assert want[j].tobytes() == cases.expected_proof(rows[j]).tobytes()


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130])
def test_assemble_many_equals_assemble(params, table, k):
    lib = _lib.load()
    idx, sums, r, s, want = _pick(table, k)
    out = np.full((k + 1, 48), SENTINEL, dtype=np.uint64)
    rcs = np.full(k + 1, -77, dtype=np.int32)
    assert lib.bh_groth16_assemble_many(params._h, _p(sums), _p(r), _p(s), k, _p(out), _p(rcs)) == 0
    assert not rcs[:k].any() and rcs[k] == -77 and (out[k] == SENTINEL).all()   # nothing past the k slots
    bad = [int(idx[j]) for j in range(k) if out[j].tobytes() != want[j].tobytes()]
    assert not bad, bad
    host = np.full((k, 48), SENTINEL, dtype=np.uint64)
    hrcs = np.full(k, -77, dtype=np.int32)
    assert lib.bh_test_proof_finish_host(params._h, _p(sums), _p(r), _p(s), k, _p(host), _p(hrcs)) == 0
    assert host.tobytes() == want.tobytes() and not hrcs.any()


def test_python_entry_and_k_zero(params, table):
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    rows = table[0][:3]
    got = pg.assemble_many(params, [cases.sums_record(row) for row in rows], [row["r"] for row in rows], [row["s"] for row in rows])
    for j, row in enumerate(rows):
        one = pg.assemble(params, cases.sums_record(row), row["r"], row["s"])
        assert (got[j].a.tobytes(), got[j].b.tobytes(), got[j].c.tobytes()) == (one.a.tobytes(), one.b.tobytes(), one.c.tobytes())
    assert pg.assemble_many(params, [], [], []) == []
    out = np.full(48, SENTINEL, dtype=np.uint64)
    rcs = np.full(1, -77, dtype=np.int32)
    assert lib.bh_groth16_assemble_many(params._h, None, None, None, 0, _p(out), _p(rcs)) == 0   # k = 0 touches nothing
    assert (out == SENTINEL).all() and rcs[0] == -77
    x = np.zeros(120, dtype=np.uint64)
    assert lib.bh_groth16_assemble_many(params._h, _p(x), _p(x), None, 1, _p(out), _p(rcs)) == -2   # BH_ERR_INVALID_ARG
    assert lib.bh_groth16_assemble_many(params._h, _p(x), _p(x), _p(x), 1, _p(out), None) == -2
    assert (out == SENTINEL).all() and rcs[0] == -77


@pytest.mark.parametrize("name", ["delta_g1", "delta_g2"])
def test_identity_delta_is_every_proofs_error(worker, table, name):  # noqa: F811
    from bellman_amd import UnexpectedIdentity
    from bellman_amd import groth16 as pg

    lib = _lib.load()
    bad = _params(worker, dict(cases.KEY, **{name: 0}))
    _, sums, r, s, _ = _pick(table, 5)
    out = np.full((5, 48), SENTINEL, dtype=np.uint64)
    rcs = np.full(5, -77, dtype=np.int32)
    assert lib.bh_groth16_assemble_many(bad._h, _p(sums), _p(r), _p(s), 5, _p(out), _p(rcs)) == 0
    assert list(rcs) == [1] * 5 and not out.any()   # BH_ERR_UNEXPECTED_IDENTITY (prover.rs:320-324), all-zero slots
    one = np.full(48, SENTINEL, dtype=np.uint64)
    assert lib.bh_groth16_assemble(bad._h, _p(sums[0]), _p(r[0]), _p(s[0]), _p(one)) == 1
    with pytest.raises(UnexpectedIdentity):
        pg.assemble_many(bad, [sums[0]], [3], [4])
