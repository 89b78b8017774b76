"""The Fp products over sliced operands and the G1 mixed addition built on them, on the host (no GPU).

tests/cpp/sliced_products_check.hip compiles ff.cuh / ec.cuh for the host and compares every sliced entry point with the
unsliced one it replaces in the bucket accumulation, word for word (corner operands, every limb set, the largest lazily
reduced operands, 10 000 random pairs), and xyzz_madd_sliced with xyzz_madd on chains that take the copy, doubling and
inverse branches.  The program is built with ASan + UBSan on the host side; only when the link fails for want of the
sanitizer runtime is it built without (the test prints which build ran)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(hipcc, exe, sanitize):
    cmd = [hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd += [os.path.join(ROOT, "tests", "cpp", "sliced_products_check.hip"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _sanitizer_runtime_missing(stderr):
    """the LINK failed for want of the runtime libraries - not a diagnostic of the program under -fsanitize"""
    text = stderr.lower()
    return ("libclang_rt.asan" in text or "libclang_rt.ubsan" in text or "cannot find -lasan" in text or "cannot find -lubsan" in text) \
        and ("no such file" in text or "cannot find" in text or "cannot open" in text)


def test_sliced_products_match_unsliced_word_for_word(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "sliced_products_check.bin")
    build = _build(hipcc, exe, True)
    sanitized = True
    if build.returncode != 0 and _sanitizer_runtime_missing(build.stderr):
        sanitized = False   # this compiler ships no sanitizer runtime: the comparison itself still runs
        build = _build(hipcc, exe, False)
    assert build.returncode == 0, build.stderr[-3000:]
    print("sliced_products_check built %s sanitizers" % ("with" if sanitized else "WITHOUT"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "sliced products: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
