"""Parameters::verify_step in the C++ mirror (bellman_amd/csrc/groth16.hpp) from a standalone C++ program
(tests/cpp/phase2_cubic.cpp): from a powers-of-tau transcript, rescale_delta, the step check passes, and three tampered
sets fail with the expected bit."""

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.pyref import bls12_381 as bls  # noqa: E402
from tests.test_verifier_cpu import g1_rec, g2_rec  # noqa: E402

BIN = os.path.join(ROOT, "tests", "cpp", "phase2_cubic.bin")


def _build():
    from bellman_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = os.path.join(ROOT, "bellman_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "phase2_cubic.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", BIN, os.path.join(lib, "libbellman_groth16.a"), "-L" + lib,
                           "-lbellman_hip", "-Wl,-rpath," + lib])


def test_cpp_phase2_example_builds():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_verify_step_passes_and_catches_tampering(tmp_path):
    _build()
    f = tmp_path / "gens.bin"
    f.write_bytes(g1_rec(bls.G1.gen) + g2_rec(bls.G2.gen))
    r = subprocess.run([BIN, str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.strip() == "phase2 ok"
