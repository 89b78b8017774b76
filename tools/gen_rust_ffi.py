"""Generates shim/bellman-hip/src/ffi.rs - the Rust `extern "C"` block - from include/bellman_hip.h so the
two cannot drift (tests/test_shim_cpu.py regenerates and compares).  No Rust toolchain exists in this image:
the output is checked structurally here and compiled by whoever applies the shim.

Usage: python tools/gen_rust_ffi.py [--check]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bellman_amd import _abi  # noqa: E402  (the parse of the header; makes no HIP call)

OUT = os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")

SCALAR = {
    "int": "c_int", "unsigned": "c_uint", "unsigned int": "c_uint", "long": "c_long", "uint32_t": "u32", "uint64_t": "u64",
    "int32_t": "i32", "size_t": "usize", "float": "f32", "double": "f64", "char": "c_char", "void": "c_void",
}


def rust_name(cname):
    """bh_msm_many_job -> BhMsmManyJob, bh_ctx_info_t -> BhCtxInfo"""
    return "".join(w.capitalize() for w in (cname[:-2] if cname.endswith("_t") else cname).split("_"))


def c_type_to_rust(ctype):
    """'const uint64_t *' -> '*const u64' ; 'bh_bases **' -> '*mut *mut BhBases'"""
    const, base, levels = _abi.split_type(ctype)
    r = SCALAR[base] if base in SCALAR else rust_name(base)
    if not levels:
        return r
    # the pointee of level k is const when the qualifier to its left says so: the base's `const` for the innermost
    # pointer, the `const` after the previous `*` for the others ("bh_ctx *const *": pointer to const pointer to BhCtx ->
    # *const *mut BhCtx); an unqualified outer pointer is an out-parameter
    for q in [const] + levels[:-1]:
        r = ("*const " if q else "*mut ") + r
    return r


def const_type(name, c):
    """the literal decides: unsuffixed -> c_int, `u` -> u32; a *_BYTES constant is a size"""
    return "usize" if name.endswith("_BYTES") else "u32" if c.unsigned else "c_int"


RUST_KEYWORDS = {"type", "in", "ref", "box", "move", "fn", "as", "loop", "match", "where", "use", "mod"}


def render(header):
    lines = [
        "//! `extern \"C\"` declarations of libbellman_hip - GENERATED from include/bellman_hip.h by",
        "//! tools/gen_rust_ffi.py; do not edit.  One item per C entry point, same order, same argument names.",
        "#![allow(non_camel_case_types, dead_code)]",
        "use std::os::raw::{c_char, c_int, c_long, c_uint, c_void};",
        "",
    ]
    for c in header.opaque:
        lines += ["/// opaque `%s`" % c, "#[repr(C)]", "pub struct %s {" % rust_name(c), "    _private: [u8; 0],", "}"]
    for c, fields in header.structs.items():
        plain = not any("*" in t for _, t in fields)
        lines += ["/// `%s` (include/bellman_hip.h)" % c, "#[repr(C)]",
                  "#[derive(Clone, Copy%s)]" % (", Default, Debug" if plain else ""), "pub struct %s {" % rust_name(c)]
        lines += ["    pub %s: %s," % (f, c_type_to_rust(t)) for f, t in fields] + ["}"]
    lines.append("")
    lines += ["pub const %s: %s = %s;" % (k, const_type(k, c), c.text) for k, c in header.constants.items()]
    lines += ["", "#[link(name = \"bellman_hip\")]", "extern \"C\" {"]
    for fn in header.functions:
        ps = ", ".join("%s: %s" % (("r#" + p) if p in RUST_KEYWORDS else p, c_type_to_rust(t)) for p, t in fn.params)
        lines.append("    pub fn %s(%s)%s;" % (fn.name, ps, (" -> " + c_type_to_rust(fn.ret)) if fn.ret != "void" else ""))
    lines += ["}", ""]
    return "\n".join(lines)


def main():
    out = render(_abi.PRODUCT)
    n = len(_abi.PRODUCT.functions)
    if "--check" in sys.argv:
        cur = open(OUT).read()
        if cur != out:
            print("shim/bellman-hip/src/ffi.rs is stale: run python tools/gen_rust_ffi.py")
            sys.exit(1)
        print("ffi.rs matches include/bellman_hip.h (%d entry points)" % n)
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write(out)
    print("wrote %s (%d entry points)" % (OUT, n))


if __name__ == "__main__":
    main()
