"""The kernels of the Groth16 verifier, each on its own (run with `pytest -m gpu` on a MI355X): csrc/pairing_kernels.cuh as
the product compiles it, launched by the shipped launch functions through the hooks bh_test_pairing_* and compared word for
word with tests/models/pairing_stage_model.py (tests/test_pairing_stage_model_cpu.py pins that model and the operand
tables).

What counts as equal: field values as residues mod p after Montgomery decoding; every Fp coefficient of a line or an Fp12
value below 2p; Fr results below q; affine outputs canonical; identities all-zero records; what lies past n and every
guard still the sentinel.  No tolerance anywhere: integer work.

What has run on an MI355X, and how long the file takes there: profiles/pairing_stage_gputests.txt."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import field_model as fm  # noqa: E402
from tests import group_model as gm  # noqa: E402
from tests.models import pairing_stage_model as psm  # noqa: E402

P, Q = psm.P, psm.Q
LINE_BYTES, F12_BYTES, PROOF_BYTES, LINES = 288, 576, 384, psm.MILLER_LINES
LINE_LIKE = (fm.F2_ZERO,) * 3


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


def out(nbytes):
    return np.zeros(max(nbytes, 1), dtype=np.uint8)


def call(fn, names, *args):
    """the hook with a guard array appended; asserts the return code and every guard"""
    guards = np.zeros(len(names), dtype=np.uint32)
    rc = fn(*args, guards.ctypes.data)
    assert rc == 0, rc
    for name, ok in zip(names, guards):
        assert ok == 1, "bytes behind %s were written" % name


def u32s(values):
    return psm.to_u32(values).tobytes()


def lazy_mask(k):
    """which coefficients of record k are written as v + p"""
    return (0x9249249249249249 << (k % 3)) & ((1 << 64) - 1) if k % 2 else 0


def test_shape(lib):
    s = np.zeros(16, dtype=np.uint64)
    assert lib.bh_test_pairing_stage_shape(s.ctypes.data) == 0
    assert list(s) == [LINE_BYTES, F12_BYTES, PROOF_BYTES, LINES, psm.PF_IDENTITY, psm.PF_OFF_CURVE, psm.PT_INVALID_MASK,
                       psm.PT_IS_INF, psm.COLSUM_THREADS, psm.COLSUM_BLOCKS, 16384, 4096, psm.SENTINEL, 96, 288, 96]


def test_arguments_outside_a_buffer_are_refused(lib, worker):
    g = np.zeros(8, dtype=np.uint32)
    b = bytes(4096)
    ctx = worker.ctx
    assert lib.bh_test_pairing_lines_dev(ctx, b, 200, 0, 1, b, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_lines_dev(ctx, b, 192, 0, 0, b, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_ic_table_dev(ctx, b, 1, 3, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_ic_accumulate_dev(ctx, b, 1, 0, b, 16, b, 1, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_ic_accumulate_dev(ctx, b, 1, 0, None, 8, b, 1, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_colsum_dev(ctx, b, b, 1, 0, 1, 65, b, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_colsum_dev(ctx, b, b, 1, 2, 1, 0, b, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_miller3_dev(ctx, b, b, b, b, b, b, b, 0, 8, 1, b, g.ctypes.data) == -2
    assert lib.bh_test_pairing_miller_dev(ctx, b, None, None, 1, None, None, 0, b, g.ctypes.data) == -2


# ---------------------------------------------------------------------------------------------------------------- lines
def run_lines(lib, worker, points, stride, negate):
    n = len(points)
    if stride == 192:
        recs = b"".join(psm.g2_rec(q) for q in points)
    else:   # proofs: A and C are other lanes' business; here they hold the sentinel
        fill = bytes([psm.SENTINEL]) * 96
        recs = b"".join(fill + psm.g2_rec(q) + fill for q in points)
    lines, flags = out(n * LINES * LINE_BYTES), np.zeros(n, dtype=np.uint32)
    call(lib.bh_test_pairing_lines_dev, ("records", "lines", "flags"), worker.ctx, recs, stride, negate, n, lines.ctypes.data,
         flags.ctypes.data)
    return lines, flags


def check_lines(points, negate, lines, flags, tag):
    for i, q in enumerate(points):
        raw = lines[i * LINES * LINE_BYTES:(i + 1) * LINES * LINE_BYTES].tobytes()
        if q is None:
            assert flags[i] == psm.PF_IDENTITY and psm.is_sentinel(raw), (tag, i)
            continue
        assert flags[i] == (0 if gm.on_curve(2, q) else psm.PF_OFF_CURVE), (tag, i)
        want = psm.g2_lines(gm.neg(2, q) if negate else q)
        assert psm.decode_lazy(raw, (LINE_LIKE,) * LINES) == want, (tag, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lines(lib, worker, n):
    plan, rotations = psm.lane_plan(psm.g2_points(), n)
    for rot in range(rotations):
        points = [pt for _, pt in plan(rot)]
        for stride, negate in [(s, g) for s in (192, 384) for g in (0, 1)]:   # every class at the hot lanes under every pair
            lines, flags = run_lines(lib, worker, points, stride, negate)
            check_lines(points, negate, lines, flags, (n, rot, stride, negate))


# --------------------------------------------------------------------------------------------------------------- miller
def miller_operands(n, tag):
    """n (P, Q) pairs: every G1 class against a few G2 points, identities of Q among them"""
    g1, g2 = psm.g1_points(), psm.g2_points()
    ps = [pt for name in sorted(g1) for pt in g1[name]]
    qs = [g2["generator"][0], g2["random"][0], None, g2["off_subgroup"][0], g2["off_curve"][0]]
    rot = len(tag)
    return [(ps[(j + rot) % len(ps)], qs[(j // 2 + rot) % len(qs)]) for j in range(n)]


def lines_and_flags(qs, first):
    """model lines (every other record with lazily reduced coefficients); an identity keeps the sentinel and its flag"""
    recs, flags = [], []
    for k, q in enumerate(qs):
        if q is None:
            recs.append(bytes([psm.SENTINEL]) * (LINES * LINE_BYTES))
            flags.append(psm.PF_IDENTITY)
        else:
            recs.append(psm.lines_rec(psm.g2_lines(q), lazy_mask(first + k)))
            flags.append(0 if gm.on_curve(2, q) else psm.PF_OFF_CURVE)
    return b"".join(recs), flags


def run_miller(lib, worker, ps, l0, f0, n0, l1, f1, n1):
    n = n0 + n1
    f = out(n * F12_BYTES)
    call(lib.bh_test_pairing_miller_dev, ("p", "lines0", "flags0", "lines1", "flags1", "f"), worker.ctx,
         b"".join(psm.g1_rec(p) for p in ps), l0 if n0 else None, u32s(f0) if n0 else None, n0, l1 if n1 else None,
         u32s(f1) if n1 else None, n1, f.ctypes.data)
    return f


def f12_at(buf, i):
    return psm.decode_lazy(buf[i * F12_BYTES:(i + 1) * F12_BYTES].tobytes(), fm.F12_ONE)


@pytest.mark.parametrize("n0,n1", [(1, 0), (0, 3), (1, 3), (64, 3), (65, 3), (130, 0)])
def test_miller(lib, worker, n0, n1):
    pairs = miller_operands(n0 + n1, "x" * (n0 % 7))
    if n0 and n1:   # an identity Q on either side of the split, a pair that is none right behind it
        pairs[n0 - 1] = (pairs[n0 - 1][0], None)
        pairs[n0] = (psm.g1_points()["random"][0], psm.g2_points()["generator"][0])
        pairs[n0 + 1] = (psm.g1_points()["generator"][0], None)
    ps, qs = [p for p, _ in pairs], [q for _, q in pairs]
    l0, f0 = lines_and_flags(qs[:n0], 0)
    l1, f1 = lines_and_flags(qs[n0:], n0)
    f = run_miller(lib, worker, ps, l0, f0, n0, l1, f1, n1)
    for i, (p, q) in enumerate(pairs):
        assert f12_at(f, i) == psm.miller(p, q), (n0, n1, i)
    if n0 and n1:
        assert f12_at(f, n0 - 1) == fm.F12_ONE and f12_at(f, n0 + 1) == fm.F12_ONE and f12_at(f, n0) != fm.F12_ONE


def test_miller_over_the_lines_stage_output(lib, worker):
    """the raw lines of g2_lines_kernel (lazily reduced as they come) into miller_kernel, split 3 + 2"""
    g1, g2 = psm.g1_points(), psm.g2_points()
    qs = [g2["generator"][0], None, g2["random"][1], g2["x_c0_zero"][0], g2["off_curve"][0]]
    ps = [g1["random"][0], g1["generator"][0], g1["order3"][0], g1["off_subgroup"][0], g1["off_curve"][0]]
    lines, flags = run_lines(lib, worker, qs, 192, 0)
    cut = 3 * LINES * LINE_BYTES
    f = run_miller(lib, worker, ps, lines[:cut].tobytes(), flags[:3], 3, lines[cut:].tobytes(), flags[3:], 2)
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert f12_at(f, i) == psm.miller(p, q), i


# ----------------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 16385])
def test_fold(lib, worker, m):
    rnd = psm.rng("fold %d" % m)
    distinct = [psm.random_f12_lazy(rnd) for _ in range(min(m, 67))]
    raws = [distinct[(i * 29) % len(distinct)] for i in range(m)]
    buf = np.frombuffer(b"".join(psm.fp_bytes(v) for raw in raws for v in raw), dtype=np.uint8).copy()
    call(lib.bh_test_pairing_fold_dev, ("f",), worker.ctx, buf.ctypes.data, m)
    want = fm.F12_ONE
    counts = {}
    for i in range(m):
        counts[(i * 29) % len(distinct)] = counts.get((i * 29) % len(distinct), 0) + 1
    for k, c in counts.items():
        want = fm.f12_mul(want, fm.f12_pow(psm.f12_of_raw(distinct[k]), c))
    assert f12_at(buf, 0) == want, m
    # the upper half is read only: launch_fold writes f[i] for i < ceil(m / 2) at most
    h = (m + 1) // 2
    assert buf[h * F12_BYTES:].tobytes() == b"".join(psm.fp_bytes(v) for raw in raws[h:] for v in raw)


# ----------------------------------------------------------------------------------------------------------- proof_prep
def run_prep(lib, worker, proofs, z_raw, fmt, want_c):
    n = len(proofs)
    recs = b"".join(psm.proof_rec(a, gm.GEN[2], c) for a, c in proofs)
    p_out, c_out, zc_out, flags = out(n * 96), out(n * 96), out(n * 32), np.zeros(n, dtype=np.uint32)
    call(lib.bh_test_pairing_proof_prep_dev, ("proofs", "z", "generator", "p_out", "c_out", "zc_out", "flags"), worker.ctx, recs,
         None if z_raw is None else psm.fr_bytes(z_raw), fmt, n, int(want_c), psm.g1_rec(gm.GEN[1]) if want_c else None,
         p_out.ctypes.data, c_out.ctypes.data if want_c else None, zc_out.ctypes.data if want_c else None, flags.ctypes.data)
    return p_out, c_out, zc_out, flags


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("fmt", [psm.CANONICAL, psm.MONT])
def test_proof_prep(lib, worker, n, fmt):
    g1 = psm.g1_points()
    pts = [pt for name in sorted(g1) for pt in g1[name]]
    for shape, (with_z, want_c) in enumerate([(True, True), (True, False), (False, False), (False, True)]):
        # A walks the classes lane by lane, C three times as slowly: every (A, C) pair of classes within 65 lanes' reach
        proofs = [(pts[(j + shape) % len(pts)], pts[(j // 3 + 2 * shape + n) % len(pts)]) for j in range(n)]
        z_int, z_raw = psm.z_values(fmt, n, "%d %d" % (n, shape))
        p_out, c_out, zc_out, flags = run_prep(lib, worker, proofs, z_raw if with_z else None, fmt, want_c)
        for j, (a, c) in enumerate(proofs):
            tag = (n, fmt, shape, j)
            off = (a is not None and not gm.on_curve(1, a)) or (c is not None and not gm.on_curve(1, c))
            assert flags[j] == (psm.PF_OFF_CURVE if off else 0), tag
            got = psm.decode_g1(p_out[j * 96:(j + 1) * 96])
            assert got == (psm.g1_mul(a, z_int[j]) if with_z and a is not None else a), tag
            if want_c:
                assert psm.decode_g1(c_out[j * 96:(j + 1) * 96]) == (gm.GEN[1] if c is None else c), tag
                zc = psm.words(zc_out[j * 32:(j + 1) * 32], 32)[0]
                assert zc == (0 if c is None else z_raw[j] if with_z else 1), tag


# ----------------------------------------------------------------------------------------------------------- g1_mul_one
def test_g1_mul_one(lib, worker):
    g1 = psm.g1_points()
    rnd = psm.rng("mul one")
    for pt in (None, g1["generator"][0], g1["random"][1]):
        for k in (0, 1, Q - 1, rnd.randrange(Q)):
            res = out(96)
            call(lib.bh_test_pairing_g1_mul_one_dev, ("p", "s", "out"), worker.ctx, psm.g1_rec(pt),
                 psm.fr_bytes([psm.scalar_raw(k, psm.MONT)]), res.ctypes.data)
            assert psm.decode_g1(res) == (None if pt is None else psm.g1_mul(pt, k)), (pt is None, k)


# --------------------------------------------------------------------------------------------------------------- colsum
def colsum_case(lib, worker, n, ncol, fmt, nb_override=0):
    rnd = psm.rng("colsum %d %d %d" % (n, ncol, fmt))
    edges = [v for v in psm.FR_EDGES if fmt == psm.CANONICAL or v < Q]
    pool = [psm.scalar_raw(v, fmt) for v in edges] + [rnd.randrange(Q if fmt == psm.MONT else 1 << 256) for _ in range(89)]
    zpool = [r for r in pool if psm.scalar_int(r, fmt) % Q]                       # z is never 0 mod q
    z = [zpool[(j * 5) % len(zpool)] for j in range(n)]
    rows = [[pool[(j * 7 + i * 13) % len(pool)] for i in range(ncol - 1)] for j in range(n)]
    acc0 = [rnd.randrange(Q) for _ in range(ncol)]
    table = np.frombuffer(psm.fr_bytes(pool), dtype=np.uint8).reshape(len(pool), 32)
    idx = (np.arange(n)[:, None] * 7 + np.arange(ncol - 1)[None, :] * 13) % len(pool)
    acc = np.frombuffer(psm.fr_bytes(v * psm.RQ % Q for v in acc0), dtype=np.uint8).copy()
    part = out(ncol * psm.COLSUM_BLOCKS * 32)
    call(lib.bh_test_pairing_colsum_dev, ("z", "inputs", "part", "acc"), worker.ctx, psm.fr_bytes(z),
         table[idx].tobytes() if ncol > 1 else None, ncol - 1, fmt, n, nb_override, acc.ctypes.data, part.ctypes.data)
    nb = nb_override or psm.colsum_nb(n)
    want_part, want_acc = psm.colsum(z, rows, ncol, acc0, fmt, nb)
    got_acc, got_part = psm.words(acc, 32), psm.words(part, 32)
    tag = (n, ncol, fmt, nb)
    assert all(v < Q for v in got_acc) and [v * fm.RQ_INV % Q for v in got_acc] == want_acc, tag
    for col in range(ncol):
        vals = got_part[col * nb:(col + 1) * nb]
        assert all(v < Q for v in vals) and [v * fm.RQ_INV % Q for v in vals] == want_part[col], (tag, col)
    assert psm.is_sentinel(part[ncol * nb * 32:]), tag


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 16383, 16384])
def test_colsum_sizes(lib, worker, n):
    for ncol in (2, 17):
        colsum_case(lib, worker, n, ncol, psm.CANONICAL)
    colsum_case(lib, worker, n, 2, psm.MONT)


@pytest.mark.parametrize("ncol", [1, 2, 17, 65])
def test_colsum_columns(lib, worker, ncol):
    colsum_case(lib, worker, 257, ncol, psm.CANONICAL)
    colsum_case(lib, worker, 257, ncol, psm.MONT)
    colsum_case(lib, worker, 16384 if ncol < 65 else 4097, ncol, psm.CANONICAL)


def test_colsum_one_block_row_strides_over_the_proofs(lib, worker):
    colsum_case(lib, worker, 1000, 3, psm.CANONICAL, nb_override=1)
    colsum_case(lib, worker, 16384, 2, psm.MONT, nb_override=3)


# ------------------------------------------------------------------------------------------------------------- ic_table
def table_rec(table):
    return b"".join(psm.g1_rec(e) for rows in table for row in rows for e in row)


@pytest.mark.parametrize("w", psm.WIDTHS)
@pytest.mark.parametrize("n_in", [1, 3])
def test_ic_table(lib, worker, w, n_in):
    g1 = psm.g1_points()
    ic = [g1["random"][0]] if n_in == 1 else [None, (0, 2), g1["random"][1]]
    res = out(psm.table_bytes(n_in, w))
    call(lib.bh_test_pairing_ic_table_dev, ("ic", "table"), worker.ctx, b"".join(psm.g1_rec(pt) for pt in ic), n_in, w,
         res.ctypes.data)
    want = [e for rows in psm.ic_table(ic, w) for row in rows for e in row]
    assert len(want) * 96 == len(res)
    for t, e in enumerate(want):
        assert psm.decode_g1(res[t * 96:(t + 1) * 96]) == e, (w, n_in, t)


# -------------------------------------------------------------------------------------------------------- ic_accumulate
def run_accumulate(lib, worker, rows_raw, fmt, table, w, ic0):
    n, n_inputs = len(rows_raw), len(rows_raw[0])
    res = out(n * 96)
    call(lib.bh_test_pairing_ic_accumulate_dev, ("inputs", "table", "ic0", "out"), worker.ctx,
         psm.fr_bytes(v for row in rows_raw for v in row) if n_inputs else None, n_inputs, fmt,
         table_rec(table) if n_inputs else None, w, psm.g1_rec(ic0), n, res.ctypes.data)
    return [res[j * 96:(j + 1) * 96] for j in range(n)]


@pytest.mark.parametrize("w", psm.WIDTHS)
def test_ic_accumulate(lib, worker, w):
    g1 = psm.g1_points()
    ic1, ic3 = g1["random"][0], g1["random"][1]
    rnd = psm.rng("accumulate")                              # (the same scalars at every width: the model's multiples are shared)
    some = {fmt: [rnd.randrange(Q if fmt == psm.MONT else 1 << 256) for _ in range(6)] for fmt in (psm.CANONICAL, psm.MONT)}
    keys = {   # name -> (ic_0, [ic_1, ic_2, ic_3])
        "plain": (g1["generator"][0], [ic1, g1["random"][2], ic3]),
        "identity ic_0 and ic_2": (None, [ic1, None, ic3]),
        "ic_2 = ic_1": (None, [ic1, ic1, None]),
        "ic_2 = -ic_1": (None, [ic1, gm.neg(1, ic1), None]),
    }
    for name, (ic0, ic) in keys.items():
        table = psm.ic_table(ic, w)
        for fmt in (psm.CANONICAL, psm.MONT):
            edges = [v for v in psm.FR_EDGES if fmt == psm.CANONICAL or v < Q]
            for n in (1, 64, 65) if name == "plain" else (65,):
                rows = []
                for j in range(n):
                    a = edges[j % len(edges)] if j < 2 * len(edges) else some[fmt][j % 6]
                    b = a if name.startswith("ic_2") or j % 2 else edges[(j // 2) % len(edges)]
                    rows.append((a, b, edges[(j // 3) % len(edges)] if j % 4 else some[fmt][(j // 4) % 6]))
                if name == "ic_2 = ic_1":
                    rows[0] = (1, 1, 0)                      # the second term meets an accumulator equal to it
                got = run_accumulate(lib, worker, [[psm.scalar_raw(v, fmt) for v in row] for row in rows], fmt, table, w, ic0)
                for j, row in enumerate(rows):
                    want = psm.ic_accumulate(ic0, ic, row)
                    assert psm.decode_g1(got[j]) == want, (w, name, fmt, n, j)
                    if name == "ic_2 = -ic_1":
                        assert want is None and bytes(got[j]) == bytes(96), (w, fmt, j)


@pytest.mark.parametrize("w", psm.WIDTHS)
def test_ic_accumulate_without_inputs(lib, worker, w):
    for ic0 in (psm.g1_points()["random"][2], None):
        got = run_accumulate(lib, worker, [[]] * 65, psm.CANONICAL, None, w, ic0)
        assert all(psm.decode_g1(g) == ic0 for g in got)


# -------------------------------------------------------------------------------------------------------------- miller3
def miller3_setup(n, tag):
    g1, g2 = psm.g1_points(), psm.g2_points()
    a_pool = [g1["random"][0], g1["generator"][0], None, g1["order3"][0], g1["off_curve"][0]]
    b_pool = [g2["generator"][0], g2["random"][0], None]
    acc_pool = [g1["random"][1], None, g1["off_subgroup"][0], g1["generator"][0]]
    c_pool = [g1["random"][2], g1["order3"][1], None]
    rot = len(tag)
    return [(a_pool[(j + rot) % 5], b_pool[(j // 2 + rot) % 3], acc_pool[(j // 3 + rot) % 4], c_pool[(j + j // 5 + rot) % 3])
            for j in range(n)]


def run_miller3(lib, worker, lanes, kq, kflags, separate, pairs):
    n = len(lanes)
    blines, bflags = lines_and_flags([b for _, b, _, _ in lanes], 1)
    klines = b"".join(psm.lines_rec(psm.g2_lines(q)) for q in kq)
    f = out((3 if separate else 1) * n * F12_BYTES)
    call(lib.bh_test_pairing_miller3_dev, ("a", "acc", "proofs", "blines", "bflags", "klines", "kflags", "f"), worker.ctx,
         b"".join(psm.g1_rec(a) for a, _, _, _ in lanes), b"".join(psm.g1_rec(g) for _, _, g, _ in lanes),
         b"".join(psm.proof_rec(None, None, c) for _, _, _, c in lanes), blines, u32s(bflags), klines, u32s(kflags),
         int(separate), pairs, n, f.ctypes.data)
    return f


def miller3_expect(lane, kq, kflags):
    a, b, g, c = lane
    return [psm.miller(a, b), psm.miller(g, None if kflags[0] & 1 else kq[0]), psm.miller(c, None if kflags[1] & 1 else kq[1])]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_miller3(lib, worker, n):
    g2 = psm.g2_points()
    kq = [gm.neg(2, g2["random"][1]), g2["generator"][0]]
    lanes = miller3_setup(n, "y" * n)
    if n == 1:
        lanes = [(psm.g1_points()["random"][0], g2["random"][0], psm.g1_points()["random"][1], psm.g1_points()["generator"][0])]
    for kflags in ([0, 0], [1, 0], [0, 1]) if n != 64 else ([0, 2],):   # (an off-curve flag of the key switches nothing off)
        want = [miller3_expect(lane, kq, kflags) for lane in lanes]
        f = run_miller3(lib, worker, lanes, kq, kflags, True, 7)
        for y in range(3):
            for j in range(n):
                assert f12_at(f, y * n + j) == want[j][y], (n, kflags, "separate", y, j)
        for pairs in (7, 1, 2, 4):
            f = run_miller3(lib, worker, lanes, kq, kflags, False, pairs)
            for j in range(n):
                assert f12_at(f, j) == psm.f12_product(want[j][y] for y in range(3) if (pairs >> y) & 1), (n, kflags, pairs, j)
    if n == 1:   # with everything switched on, no factor is 1
        assert all(v != fm.F12_ONE for v in miller3_expect(lanes[0], kq, [0, 0]))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_fold3_and_constant(lib, worker, n):
    rnd = psm.rng("fold3 %d" % n)
    const = psm.random_f12_lazy(rnd)
    for separate in (1, 0):
        k = 3 if separate else 1
        distinct = [psm.random_f12_lazy(rnd) for _ in range(7)]
        raws = [distinct[(i * 3 + i // 7) % 7] for i in range(k * n)]
        buf = np.frombuffer(b"".join(psm.fp_bytes(v) for raw in raws for v in raw), dtype=np.uint8).copy()
        call(lib.bh_test_pairing_fold3_const_dev, ("f", "c"), worker.ctx, buf.ctypes.data,
             b"".join(psm.fp_bytes(v) for v in const), n, separate)
        for j in range(n):
            want = psm.f12_product([psm.f12_of_raw(raws[y * n + j]) for y in range(k)] + [psm.f12_of_raw(const)])
            assert f12_at(buf, j) == want, (n, separate, j)


# -------------------------------------------------------------------------------------------------------------- verdict
def verdict_rows():
    states = [0, psm.PT_IS_INF] + list(psm.PT_INVALID_BITS) + [psm.PT_IS_INF | 8]
    word_set = {s << (8 * pos) for s in states for pos in range(3)}
    word_set |= {(s << (8 * p1)) | (t << (8 * p2)) for s in states for t in states for p1 in range(3) for p2 in range(p1 + 1, 3)}
    rows = []
    for k, word in enumerate(sorted(word_set)):
        for pf in (0, 2):
            for qf in (0, 1, 2, 3):
                rows.append((word, pf, qf, (k + pf + qf) % 3))
    for is_one in (0, 1, 2, 0xA5A5A5A5):
        rows += [(0, pf, qf, is_one) for pf in (0, 2) for qf in (0, 1, 2, 3)]
    return rows


def test_verdict(lib, worker):
    rows = verdict_rows()
    assert {psm.verdict(*r) for r in rows} == {psm.OK, psm.INVALID_POINT, psm.POINT_AT_INFINITY, psm.INVALID_PROOF}
    n = 257
    rows += rows[:(-len(rows)) % n]
    for first in range(0, len(rows), n):
        chunk = rows[first:first + n]
        cols = [u32s(r[k] for r in chunk) for k in range(4)]
        for with_words in (True, False):
            got = np.full(n, -99, dtype=np.int32)
            call(lib.bh_test_pairing_verdict_dev, ("words", "pflags", "qflags", "is_one", "verdicts"), worker.ctx,
                 cols[0] if with_words else None, cols[1], cols[2], cols[3], n, got.ctypes.data)
            want = [psm.verdict(r[0] if with_words else None, r[1], r[2], r[3]) for r in chunk]
            assert list(got) == want, (first, with_words)


# -------------------------------------------------------------------------------------------------------- final_exp, n = 65
def test_final_exponentiation_across_a_wavefront(lib, worker):
    g1, g2 = psm.g1_points(), psm.g2_points()
    f = psm.miller(g1["generator"][0], g2["generator"][0])
    g = psm.miller(gm.neg(1, g1["generator"][0]), g2["generator"][0])
    values = [f, fm.f12_mul(f, g), fm.F12_ONE]
    want = [fm.f12_pow(v, fm.FINAL_EXP) for v in values]
    assert want[0] != fm.F12_ONE and want[1] == fm.F12_ONE
    n = 65
    picks = [j % 3 for j in range(n)]
    res, is_one = out(n * F12_BYTES), np.zeros(n, dtype=np.uint32)
    call(lib.bh_test_pairing_final_exp_dev, ("f", "out", "is_one", "workspace"), worker.ctx,
         b"".join(psm.mont_bytes(values[k], lazy_mask(j)) for j, k in enumerate(picks)), n, res.ctypes.data, is_one.ctypes.data)
    for j, k in enumerate(picks):
        assert psm.decode_lazy(res[j * F12_BYTES:(j + 1) * F12_BYTES].tobytes(), fm.F12_ONE, bound=P) == want[k], j
        assert is_one[j] == (1 if k else 0), j


# ------------------------------------------------------------------------------------- window widths through the product
def g2_arr(pt):
    return np.frombuffer(psm.g2_rec(pt), dtype=np.uint64)


def g1_arr(pt):
    return np.frombuffer(psm.g1_rec(pt), dtype=np.uint64)


@pytest.fixture(scope="module")
def width_cases():
    """a 16-input key of known discrete logs, and (proof, inputs, fmt) items: valid ones over edge scalars, corrupted ones"""
    key = psm.ScalarKey(16, "widths")
    rnd = psm.rng("width items")
    edge = [0, 1, Q - 1]
    items = []
    for j in range(12):
        ins = [edge[(j + k) % 3] if (j + k) % 4 else rnd.randrange(Q) for k in range(16)]
        proof = key.proof(ins)
        if j % 4 == 1:      # canonical values >= q name the same statement
            ins = [v + Q if (k % 3 == 0 and v + Q < 1 << 256) else v for k, v in enumerate(ins)]
        if j == 2:
            ins = ins[:15] + [(1 << 256) - 1]                 # another statement: 2^256 - 1 mod q is not ins[15]
        if j % 4 == 3:
            ins = ins[:5] + [(ins[5] + 1) % Q] + ins[6:]      # a wrong input
        if j == 8:
            proof = (proof[0], proof[1], gm.add(1, proof[2], gm.GEN[1]))   # a wrong C
        items.append((psm.proof_rec(*proof), ins))
    return key, items


def verify_each(lib, pvk, items, fmt):
    n = len(items)
    verdicts = (ctypes.c_int32 * n)(*([-99] * n))
    ins = psm.fr_bytes(psm.scalar_raw(v, fmt) for _, row in items for v in row)
    rc = lib.bh_groth16_verify_each(pvk._h, b"".join(p for p, _ in items), n, ins, 16, fmt, verdicts, None)
    assert rc == 0
    return list(verdicts)


@pytest.fixture(scope="module")
def width_reference(lib, worker, width_cases):
    """the verdicts of the 8-bit table under the context's own budget"""
    from bellman_amd import verifier

    key, items = width_cases
    pvk = verifier.PreparedVerifyingKey.from_elements(worker, g1_arr(key.alpha), g2_arr(key.beta), g2_arr(key.gamma),
                                                      g2_arr(key.delta), np.stack([g1_arr(pt) for pt in key.ic]))
    try:
        before = worker.info()["table_bytes"]
        canonical = verify_each(lib, pvk, items, psm.CANONICAL)
        assert worker.info()["table_bytes"] - before == psm.table_bytes(16, 8)
        mont_items = [(p, [v % Q for v in row]) for p, row in items]
        mont = verify_each(lib, pvk, mont_items, psm.MONT)
    finally:
        pvk.release()
    want = [psm.INVALID_PROOF if j % 4 == 3 or j in (2, 8) else psm.OK for j in range(len(items))]
    assert canonical == want and psm.OK in want and psm.INVALID_PROOF in want
    return canonical, mont


@pytest.mark.parametrize("w,zero_budget", [(8, False), (4, False), (2, False), (1, False), (1, True)])
def test_window_width_chosen_by_the_table_budget(lib, worker, width_cases, width_reference, w, zero_budget):
    from bellman_amd import verifier

    key, items = width_cases
    start = worker.info()["table_bytes"]
    pvk = verifier.PreparedVerifyingKey.from_elements(worker, g1_arr(key.alpha), g2_arr(key.beta), g2_arr(key.gamma),
                                                      g2_arr(key.delta), np.stack([g1_arr(pt) for pt in key.ic]))
    info = worker.info()
    budget, before = info["table_budget"], info["table_bytes"]
    try:
        worker.set_limits(table_budget_bytes=0 if zero_budget else before + psm.table_bytes(16, w))
        canonical = verify_each(lib, pvk, items, psm.CANONICAL)
        assert worker.info()["table_bytes"] - before == psm.table_bytes(16, w), "not the %d-bit table" % w
        mont = verify_each(lib, pvk, [(p, [v % Q for v in row]) for p, row in items], psm.MONT)
        assert (canonical, mont) == width_reference, w
    finally:
        pvk.release()
        worker.set_limits(table_budget_bytes=budget)
    info = worker.info()
    assert info["table_budget"] == budget and info["table_bytes"] == start
