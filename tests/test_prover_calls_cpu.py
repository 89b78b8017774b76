"""The Groth16 prover host layer against a fake C ABI (tests/cpp/prover_calls.cpp): the sequence of C-ABI calls of every
prover path, and the outcome and the clean-up when each of those calls fails in turn, equal the record in
tests/cpp/prover_calls.expected.txt.  The record was made by the same program in two parts: lines 1-1328 (host witnesses)
from the prover as it stood before its paths were put on one table of the eight multiexps; from line 1329 (the "dev ..."
scenarios: prove_witness_batch_dev_codes over witnesses in device memory, bh_proof_finish_dev) from the prover as it stood
before the grouped bodies of its two batch entries were folded into one and moved to csrc/groth16_batch.cpp.  Both parts
are data, never regenerated from later code.  Run twice: as built by default, and with every source under ASan + UBSan (a
stand-alone program, nothing preloaded)."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXPECTED = os.path.join(CPP, "prover_calls.expected.txt")


def _archive():
    from bellman_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


@pytest.mark.parametrize("target", ["prover_calls.bin", "prover_calls_san.bin"])
def test_prover_call_sequence_and_unwind(target):
    _archive()
    build = subprocess.run(["make", "-C", CPP, "-j5", target], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-1500:] + build.stderr[-3000:]
    out = subprocess.run([os.path.join(CPP, target), EXPECTED], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "match" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
