"""The split-scalar point multiplier on the host (no GPU): the constants of bellman_amd/csrc/glv.cuh, the endomorphism
on the Python reference's points, glv_split against divmod, and the joint ladder through the host build of the text the
kernels compile (bh_test_glv_split_host, bh_test_glv_ladder_host).  Every comparison is an equality of integers or of
records.  profiles/point_mul_mutants.md lists the one-line mutants of glv.cuh these cases catch."""

import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from bellman_amd import _lib
from oracle import cref
from oracle.pyref import bls12_381 as bls
from tests.models import glv_model as model
from tests.test_compressed_cpu import header_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bellman_amd", "csrc", "glv.cuh")
P, Q, LAM = bls.P, bls.Q, model.LAMBDA
WORDS = {1: 12, 2: 24}
CURVE = {1: bls.G1, 2: bls.G2}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _halves(vals):
    return np.frombuffer(b"".join(v.to_bytes(16, "little") for v in vals), dtype=np.uint64).copy()


def _split_host(lib, ks):
    n = len(ks)
    k = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in ks), dtype=np.uint64).copy()
    k1, k2 = np.zeros(2 * n, dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64)
    lib.bh_test_glv_split_host(_p(k), _p(k1), _p(k2), n)
    return [(cref.limbs_to_int(k1[2 * i:2 * i + 2]), cref.limbs_to_int(k2[2 * i:2 * i + 2])) for i in range(n)]


def _ladder_host(lib, group, points, pairs):
    n = len(pairs)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(n, WORDS[group])
    out = np.zeros_like(pts)
    assert lib.bh_test_glv_ladder_host(group, _p(pts), _p(_halves([a for a, _ in pairs])), _p(_halves([b for _, b in pairs])), n,
                                       _p(out)) == 0
    return out


# ---- the model's own identities ------------------------------------------------------------------------------------------
def test_model_identities():
    assert LAM == 0xAC45A4010001A40200000000FFFFFFFF and LAM.bit_length() == 128
    assert LAM * LAM + LAM + 1 == Q
    assert (model.BETA ** 3) % P == 1 and model.BETA != 1 and (model.BETA2 + model.BETA + 1) % P == 0
    for k in model.corner_scalars():
        k1, k2 = model.split(k)
        assert 0 <= k1 < LAM and 0 <= k2 <= LAM + 1 and k1 + k2 * LAM == k and max(k1, k2) < 1 << 128
    assert model.split(Q - 1) == (0, LAM + 1)
    # one Barrett correction is enough below 2^255, and the corner list holds scalars that need it and that do not
    need = [k // LAM - ((k * model.MU) >> 256) for k in model.corner_scalars()]
    assert set(need) == {0, 1}


# ---- the endomorphism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_psi_is_multiplication_by_lambda(group):
    curve = CURVE[group]
    rnd = random.Random(40 + group)
    for e in (1, 2, rnd.randrange(1, Q), rnd.randrange(1, Q)):
        pt = curve.mul(curve.gen, e)
        entries = model.table(group, pt)
        assert curve.on_curve(entries[(0, 1)]) and entries[(0, 1)] == curve.mul(pt, LAM)
        assert entries[(1, 1)] == curve.add(pt, entries[(0, 1)]) == curve.mul(pt, LAM + 1)
        # the other cube root is the other eigenvalue, lambda^2: the swap is a different map
        other = model.BETA if model.PSI[group] == model.BETA2 else model.BETA2
        x = pt[0]
        wrong = (other * x % P if group == 1 else (other * x[0] % P, other * x[1] % P), pt[1])
        assert wrong == curve.mul(pt, LAM * LAM % Q) != entries[(0, 1)]


def _words(name, count):
    text = open(HEADER).read()
    body = text[text.index("static constexpr u32 %s(" % name):]
    body = body[body.index("{", body.index("constexpr u32 m")):body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{8})u", body)]
    assert len(words) == count
    return sum(w << (32 * i) for i, w in enumerate(words))


def test_header_constants_are_what_p_gives():
    assert _words("lambda", 4) == bls.BLS_X ** 2 - 1
    assert _words("mu", 5) == (1 << 256) // LAM
    rinv = pow(1 << 384, -1, P)
    beta = _words("beta", 12) * rinv % P
    assert beta == pow(2, (P - 1) // 3, P) == header_constants()[0]   # EndoConsts::beta of point_read.cuh
    assert _words("beta2", 12) * rinv % P == beta * beta % P
    # which root each group's psi takes: the header's switches against the model's table (checked against [lambda] above)
    text = open(HEADER).read()
    flags = re.findall(r"struct GlvField<(\w+)> \{.*?PSI_IS_BETA2 = (true|false);", text, flags=re.S)
    assert dict(flags) == {"FpOps": "true" if model.PSI[1] == model.BETA2 else "false",
                           "Fp2Ops": "true" if model.PSI[2] == model.BETA2 else "false"}


# ---- the split -------------------------------------------------------------------------------------------------------------
def test_split_equals_divmod(lib):
    rnd = random.Random(0x61F)
    ks = model.corner_scalars() + [rnd.randrange(Q) for _ in range(10000)]
    assert all(k < Q for k in ks)
    got = _split_host(lib, ks)
    bad = [(hex(k), g) for k, g in zip(ks, got) if g != model.split(k)]
    assert not bad, bad[:3]


# ---- the ladder ------------------------------------------------------------------------------------------------------------
def _points(group, n, seed):
    return cref.gen_bases(group, n, a=seed, b=2 * seed + 1)


@pytest.mark.parametrize("group", [1, 2])
def test_ladder_on_canonical_splits_equals_the_oracle(lib, group):
    rnd = random.Random(7 * group)
    ks = model.corner_scalars() + [rnd.randrange(Q) for _ in range(8)]
    pts = _points(group, len(ks), 11 + group)
    got = _ladder_host(lib, group, pts, [model.split(k) for k in ks])
    for i, k in enumerate(ks):
        assert got[i].tobytes() == cref.point_mul(group, pts[i], k).tobytes(), hex(k)
    assert not got[0].any()   # k = 0, the pair (0, 0): the identity record


@pytest.mark.parametrize("group", [1, 2])
def test_ladder_takes_the_equal_and_opposite_branches(lib, group):
    cases = model.branch_pairs()
    assert sorted(c[0] for c in cases) == ["equal-01", "equal-10", "equal-11", "opposite-01", "opposite-10"]
    pts = _points(group, len(cases), 5 + group)
    got = _ladder_host(lib, group, pts, [(k1, k2) for _, k1, k2, _ in cases])
    for i, (name, k1, k2, event) in enumerate(cases):
        s, events = model.trace(k1, k2)
        assert event in events and events[0] == "copy", name   # the model's trace reaches the branch
        assert got[i].tobytes() == cref.point_mul(group, pts[i], s).tobytes(), name
    assert any(k1 >= LAM or k2 > LAM + 1 or k1 + k2 * LAM >= Q for _, k1, k2, _ in cases)   # no canonical split does this


@pytest.mark.parametrize("group", [1, 2])
def test_ladder_on_the_identity_and_on_all_one_halves(lib, group):
    top = (1 << 128) - 1
    pairs = [(3, 5), model.split(Q - 1), (top, top), (top, 0), (0, top), (0, 0)]
    pts = _points(group, len(pairs), 3)
    pts[0] = 0
    pts[1] = 0
    got = _ladder_host(lib, group, pts, pairs)
    assert not got[0].any() and not got[1].any() and not got[5].any()
    for i in (2, 3, 4):
        assert got[i].tobytes() == cref.point_mul(group, pts[i], model.trace(*pairs[i])[0]).tobytes()


# ---- the same text under ASan + UBSan, in a program of its own ----------------------------------------------------------------
def test_glv_host_check_under_sanitizers(tmp_path):
    """tests/cpp/glv_host_check.hip: the split over the corner scalars against a shift-and-subtract division, the ladder of
    both groups over canonical, branch-reaching and extreme pairs against the plain double-and-add ladder."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "glv_host_check.bin")
    src = os.path.join(ROOT, "tests", "cpp", "glv_host_check.hip")
    base = [hipcc, "--cuda-host-only", "-O0", "-g", "-std=c++17"]   # (-O1 under the sanitizers builds for 100 s, -O0 for 18)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    build = subprocess.run(base + san + [src, "-o", exe], capture_output=True, text=True, timeout=600)
    text = build.stderr.lower()
    if build.returncode != 0 and ("libclang_rt.asan" in text or "libclang_rt.ubsan" in text) and \
            ("no such file" in text or "cannot find" in text or "cannot open" in text):
        print("glv_host_check built WITHOUT sanitizers: this compiler ships no sanitizer runtime")
        build = subprocess.run(base + [src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "glv host check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
