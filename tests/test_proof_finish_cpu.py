"""The device proof assembly on the host (no GPU): bh_test_proof_finish_host_vk runs the host compilation of the device
functions of bellman_amd/csrc/proof_finish.cuh - the text the kernels of proof_finish.hip compile - over rows whose points
are known multiples of the generators (tests/models/proof_finish_cases.py), so the proof a row must give is
prover.rs:326-360 on three exponents.  The records are compared byte for byte: with the C oracle's points for every row,
with the Python reference's integers for three, and with the library's own host arithmetic (bh_point_mul / bh_point_add:
what bh_groth16_assemble computes with) for every row.  bh_groth16_assemble itself takes a bh_params, which exists only
with a device context: tests/test_gpu_assemble_many.py holds the hook and the kernels against it.
profiles/proof_finish_mutants.md lists the one-line mutants of proof_finish.cuh these cases catch."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bellman_amd import _lib
from bellman_amd.groth16 import fr_to_mont_array
from oracle import cref
from oracle.pyref import bls12_381 as bls
from tests.models import proof_finish_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = bls.Q


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def corner():
    return cases.corner_rows()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def finish_host(lib, rows, vk5):
    k = len(rows)
    sums = np.ascontiguousarray(np.stack([cases.sums_record(row) for row in rows]))
    r, s = fr_to_mont_array([row["r"] for row in rows]), fr_to_mont_array([row["s"] for row in rows])
    out = np.full((k, 48), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rcs = np.full(k, -77, dtype=np.int32)
    assert lib.bh_test_proof_finish_host_vk(_p(vk5), _p(sums), _p(r), _p(s), k, _p(out), _p(rcs)) == 0
    return out, rcs


def test_the_key_is_pointgens_and_the_rows_cover_the_corners(corner):
    vk = cases.key_points()
    rec = cases.key_records()
    assert cref.g1_to_py(rec["alpha_g1"])[0] == vk["alpha_g1"] and cref.g2_to_py(rec["delta_g2"])[0] == vk["delta_g2"]
    assert cref.g1_to_py(rec["beta_g1"])[0] == vk["beta_g1"] and cref.g2_to_py(rec["beta_g2"])[0] == vk["beta_g2"]
    assert cref.g1_to_py(rec["delta_g1"])[0] == vk["delta_g1"]
    assert not cases.point(1, 0).any() and not cases.point(2, Q).any()
    for name in ("r-zero", "s-zero", "both-zero", "r-q-minus-1", "r-low-half-zero", "s-high-half-zero", "all-sums-identity",
                 "a-in-equals-a-aux", "a-in-is-minus-a-aux", "A-identity", "B-identity", "h-is-minus-l", "a-aux-alone-identity",
                 "b2-in-alone-identity", "h-alone-identity"):
        assert name in corner
    assert corner["r-low-half-zero"]["r"] % cases.LAM == 0 and corner["s-high-half-zero"]["s"] < cases.LAM
    assert all(0 <= row["r"] < Q and 0 <= row["s"] < Q for row in corner.values())


def test_corner_rows_equal_the_exponent_arithmetic(lib, corner):
    names = sorted(corner)
    got, rcs = finish_host(lib, [corner[n] for n in names], cases.vk5())
    assert not rcs.any()
    bad = [n for j, n in enumerate(names) if got[j].tobytes() != cases.expected_proof(corner[n]).tobytes()]
    assert not bad, bad
    j = names.index("A-identity")
    assert not got[j][:12].any() and got[j][12:].any()
    j = names.index("B-identity")
    assert not got[j][12:36].any() and got[j][:12].any()
    j = names.index("C-identity")
    assert not got[j][36:].any() and got[j][:36].any()


def test_random_rows_equal_the_exponent_arithmetic(lib):
    rows = cases.random_rows(24, 0xF1)
    got, rcs = finish_host(lib, rows, cases.vk5())
    assert not rcs.any()
    for j, row in enumerate(rows):
        assert got[j].tobytes() == cases.expected_proof(row).tobytes(), j


def test_three_rows_against_the_python_reference(lib, corner):
    G1, G2 = bls.G1, bls.G2
    rows = [corner["a-in-equals-a-aux"], corner["rs-is-one"], cases.random_rows(1, 3)[0]]
    got, _ = finish_host(lib, rows, cases.vk5())
    vk = cases.key_points()
    for j, row in enumerate(rows):
        r, s = row["r"], row["s"]
        pt = {n: (G1 if cases.GROUP[n] == 1 else G2).mul((G1 if cases.GROUP[n] == 1 else G2).gen, row["sums"][n]) for n in cases.SLOTS}
        a_ans, b1_ans = G1.add(pt["a_in"], pt["a_aux"]), G1.add(pt["b1_in"], pt["b1_aux"])
        a = G1.add(G1.add(G1.mul(vk["delta_g1"], r), vk["alpha_g1"]), a_ans)                      # prover.rs:326-327, 339-343
        b = G2.add(G2.add(G2.mul(vk["delta_g2"], s), vk["beta_g2"]), G2.add(pt["b2_in"], pt["b2_aux"]))
        c = G1.add(G1.add(G1.mul(vk["delta_g1"], r * s % Q), G1.mul(vk["alpha_g1"], s)), G1.mul(vk["beta_g1"], r))
        c = G1.add(G1.add(c, G1.mul(a_ans, s)), G1.mul(b1_ans, r))
        c = G1.add(G1.add(c, pt["h"]), pt["l"])
        assert cref.g1_to_py(got[j][:12])[0] == a and cref.g2_to_py(got[j][12:36])[0] == b and cref.g1_to_py(got[j][36:])[0] == c


def test_rows_equal_the_librarys_host_arithmetic(lib, corner):
    """blind_terms / finish_proof of csrc/groth16_prover.cpp with the library's host group operations"""
    rec = cases.key_records()

    def mul(group, pt, k):
        out = np.zeros_like(pt)
        kc = np.array(cref.int_to_limbs(k % Q, 4), dtype=np.uint64)
        lib.bh_point_mul(group, _p(out), _p(np.ascontiguousarray(pt)), _p(kc))
        return out

    def add(group, x, y):
        out = np.zeros_like(x)
        lib.bh_point_add(group, _p(out), _p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(y)), 1)
        return out

    names = sorted(corner)
    rows = [corner[n] for n in names] + cases.random_rows(4, 17)
    got, _ = finish_host(lib, rows, cases.vk5())
    for j, row in enumerate(rows):
        r, s = row["r"], row["s"]
        m = cases.sums_record(row)
        a_in, a_aux, b1_in, b1_aux, b2_in, b2_aux, h, l = (m[0:12], m[12:24], m[24:36], m[36:48], m[48:72], m[72:96], m[96:108],
                                                            m[108:120])
        a = add(1, add(1, add(1, mul(1, rec["delta_g1"], r), rec["alpha_g1"]), a_in), a_aux)
        b = add(2, add(2, add(2, mul(2, rec["delta_g2"], s), rec["beta_g2"]), b2_in), b2_aux)
        c = add(1, add(1, mul(1, rec["delta_g1"], r * s % Q), mul(1, rec["alpha_g1"], s)), mul(1, rec["beta_g1"], r))
        for pt, k in ((a_in, s), (a_aux, s), (b1_in, r), (b1_aux, r)):
            c = add(1, c, mul(1, pt, k))
        c = add(1, add(1, c, h), l)
        assert got[j].tobytes() == np.concatenate([a, b, c]).tobytes(), names[j] if j < len(names) else j


def test_identity_delta_is_refused_for_every_row(lib):
    rows = cases.random_rows(3, 5)
    for name in ("delta_g1", "delta_g2"):
        got, rcs = finish_host(lib, rows, cases.vk5(dict(cases.KEY, **{name: 0})))
        assert list(rcs) == [1, 1, 1] and not got.any()   # BH_ERR_UNEXPECTED_IDENTITY, prover.rs:320-324


def test_arguments(lib):
    vk5 = cases.vk5()
    x = np.zeros(120, dtype=np.uint64)
    out = np.full(48, 7, dtype=np.uint64)
    rcs = np.full(1, -77, dtype=np.int32)
    assert lib.bh_test_proof_finish_host_vk(_p(vk5), None, None, None, 0, None, None) == 0   # k = 0 touches nothing
    assert lib.bh_test_proof_finish_host_vk(None, _p(x), _p(x), _p(x), 1, _p(out), _p(rcs)) == -2
    assert lib.bh_test_proof_finish_host_vk(_p(vk5), None, _p(x), _p(x), 1, _p(out), _p(rcs)) == -2
    assert lib.bh_test_proof_finish_host(None, _p(x), _p(x), _p(x), 1, _p(out), _p(rcs)) == -2
    assert lib.bh_groth16_assemble_many(None, _p(x), _p(x), _p(x), 1, _p(out), _p(rcs)) == -2
    assert (out == 7).all() and rcs[0] == -77   # BH_ERR_INVALID_ARG each time, nothing written


# ---- the same text under ASan + UBSan, in a program of its own ----------------------------------------------------------------
def test_proof_finish_host_check_under_sanitizers(tmp_path):
    """tests/cpp/proof_finish_host_check.hip: both stages of proof_finish.cuh over corner and random rows against the plain
    double-and-add ladder and the general addition."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "proof_finish_host_check.bin")
    src = os.path.join(ROOT, "tests", "cpp", "proof_finish_host_check.hip")
    base = [hipcc, "--cuda-host-only", "-O0", "-g", "-std=c++17"]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    build = subprocess.run(base + san + [src, "-o", exe], capture_output=True, text=True, timeout=600)
    text = build.stderr.lower()
    if build.returncode != 0 and ("libclang_rt.asan" in text or "libclang_rt.ubsan" in text) and \
            ("no such file" in text or "cannot find" in text or "cannot open" in text):
        print("proof_finish_host_check built WITHOUT sanitizers: this compiler ships no sanitizer runtime")
        build = subprocess.run(base + [src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "proof finish host check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
