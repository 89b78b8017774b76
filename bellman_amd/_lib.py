"""Loader of the C-ABI shared library (include/bellman_hip.h).

There is NO CPU fallback: if libbellman_hip.so is missing, or no gfx950 device is visible
when a context is requested, this raises.  The library is built in-tree by
`make -C bellman_amd/csrc` (or `__graft_entry__.build()`).
"""

import ctypes
import os
import subprocess

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# BELLMAN_HIP_LIB: another build of the SAME library (A/B runs of a kernel experiment against the shipped build, e.g.
# tools/build_variant.sh) - honoured only together with BELLMAN_HIP_ALLOW_LIB_OVERRIDE=1, so that a stray variable cannot
# swap the library under the tests or the bench (bench.py prints bh_version() and the library's path and hash into its
# JSON line).  Never a different implementation - there is no fallback of any kind.
_OVERRIDE = os.environ.get("BELLMAN_HIP_LIB") if os.environ.get("BELLMAN_HIP_ALLOW_LIB_OVERRIDE") == "1" else None
LIB_PATH = _OVERRIDE or os.path.join(_HERE, "lib", "libbellman_hip.so")

TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libbellman_hip_test.so")
# the demo circuits once more, compiled WITHOUT the closure checks of the test library (csrc/Makefile): what bench.py times
DEMO_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libbellman_hip_demo.so")
DEMO_EXPORTS = ["bh_groth16_prove_demo", "bh_groth16_demo_r1cs", "bh_groth16_prove_demo_r1cs", "bh_groth16_prove_demo_async",
                "bh_groth16_prove_demo_r1cs_part", "bh_test_synthesis_ms"]

# every symbol include/bellman_hip.h declares (libbellman_hip.so exports exactly these) ...
EXPORTS = [f.name for f in _abi.PRODUCT.functions]
# ... and what include/bellman_hip_test.h declares: test hooks and the built-in demo circuits, in libbellman_hip_test.so
TEST_EXPORTS = [f.name for f in _abi.TEST.functions]


def library_identity():
    """What was loaded: bh_version(), the path, the first 16 hex digits of the file's sha256 (bench.py's JSON line)."""
    import hashlib

    lib = load()
    with open(LIB_PATH, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    return {"version": lib.bh_version().decode(), "path": os.path.relpath(LIB_PATH, os.path.dirname(_HERE)), "sha256_16": digest,
            "override": bool(_OVERRIDE)}


def build(jobs=8):
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j%d" % jobs])
    return LIB_PATH


_lib = None


class _Libs:
    """The product library, with the test library behind it: an attribute that libbellman_hip.so does not export (a test
    hook, a demo-circuit entry point) resolves in libbellman_hip_test.so, which links against the product library."""

    def __init__(self, product, test):
        self.product, self.test = product, test
        self.demo_unchecked = None

    def use_unchecked_demo_circuits(self):
        """bench.py: the demo-circuit entry points (DEMO_EXPORTS) from libbellman_hip_demo.so - the same circuits whose
        closures do not count their terms (the checking build costs 1.5-2 % of a synthesis)."""
        if self.demo_unchecked is None:
            if not os.path.exists(DEMO_LIB_PATH):
                raise RuntimeError("libbellman_hip_demo.so not built (run `make -C bellman_amd/csrc`)")
            d = ctypes.CDLL(DEMO_LIB_PATH)
            for name in DEMO_EXPORTS:
                f = getattr(d, name)
                t = getattr(self.test, name)
                f.argtypes, f.restype = t.argtypes, t.restype
                self.__dict__[name] = f
            self.demo_unchecked = d
        return self

    def __getattr__(self, name):
        try:
            return getattr(self.product, name)
        except AttributeError:
            if self.test is None:
                raise
            return getattr(self.test, name)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libbellman_hip.so not built (run `make -C bellman_amd/csrc`); "
            "bellman_amd has no CPU fallback"
        )
    # more hardware queues than the runtime's 4: a proof runs 6-7 job streams at once (see api_context.hip); must be in the
    # environment before the process' first HIP call
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    product = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    lib = _Libs(product, ctypes.CDLL(TEST_LIB_PATH) if os.path.exists(TEST_LIB_PATH) else None)
    lib.bh_runtime_configure()   # records that the request was made before this library's first HIP call
    # every signature as the headers declare it (_abi.py): pointers are c_void_p, scalars keep their exact width
    for header, cdll in ((_abi.PRODUCT, product), (_abi.TEST, lib.test)):
        for fn in header.functions if cdll is not None else ():
            f = getattr(cdll, fn.name)
            f.argtypes, f.restype = [_abi.ctype_of(t) for _, t in fn.params], _abi.restype_of(fn.ret)
    _lib = lib
    return lib
