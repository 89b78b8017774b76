"""The Rust side of the boundary (shim/) cannot be compiled in this image (no Rust toolchain), so what can be
checked mechanically is: ffi.rs is exactly what the generator makes from include/bellman_hip.h (names,
argument names, argument count and types per entry point), the test-hook header is not bound, the constants
agree with the header, the wrapper calls only bound functions, every hunk of the patch is well formed, and the
shim's Rust files and the patch's new src/hip.rs keep their brackets balanced."""

import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PATCH = os.path.join(ROOT, "shim", "patches", "bellman-hip.patch")


def _patch_hunks():
    """The unified diff as {path: [(old_start, old_len, new_start, new_len, body lines)]}; asserts that every hunk's body
    holds exactly the old- and new-side line counts of its header and that nothing stands between hunks."""
    lines = open(PATCH).read().split("\n")
    if lines[-1] == "":
        lines.pop()
    files, path, i = {}, None, 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("diff ") or ln.startswith("--- "):
            i += 1
            continue
        if ln.startswith("+++ "):
            path = ln[4:].split("\t")[0]
            assert path.startswith("b/"), ln
            path = path[2:]
            files[path] = []
            i += 1
            continue
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", ln)
        assert m and path is not None, "line %d: %r stands outside a hunk" % (i + 1, ln)
        os_, ol, ns, nl = (int(x) if x is not None else 1 for x in m.groups())
        body, old, new = [], 0, 0
        i += 1
        while old < ol or new < nl:
            assert i < len(lines), "hunk %r of %s is truncated" % (ln, path)
            b = lines[i]
            assert b[:1] in (" ", "-", "+", "\\"), "hunk %r of %s: line %d %r" % (ln, path, i + 1, b)
            old += b[:1] in (" ", "-")
            new += b[:1] in (" ", "+")
            body.append(b)
            i += 1
        assert (old, new) == (ol, nl), "hunk %r of %s holds %d / %d lines" % (ln, path, old, new)
        while i < len(lines) and lines[i].startswith("\\"):   # "\ No newline at end of file"
            i += 1
        files[path].append((os_, ol, ns, nl, body))
    return files


def test_patch_hunks_are_well_formed():
    """No upstream tree is needed: the header counts of every hunk match its body, and within a file the hunks are in
    order, do not overlap, and each new-side start is the old-side start shifted by the lines the earlier hunks added."""
    files = _patch_hunks()
    assert {"src/hip.rs", "src/multiexp.rs", "src/domain.rs", "src/multicore.rs", "src/lib.rs", "groth16/src/prover.rs"} <= set(files)
    for path, hunks in files.items():
        assert hunks, path
        shift, end = 0, 0
        for os_, ol, ns, nl, _ in hunks:
            assert os_ >= end, (path, os_, end)
            if ol:
                assert ns == os_ + shift, (path, os_, ns, shift)
            end = os_ + ol
            shift += nl - ol
    (hip,) = files["src/hip.rs"]
    assert hip[:2] == (0, 0) and all(b.startswith("+") for b in hip[4]), "src/hip.rs is a new file"


def _strip_rust(text):
    text = re.sub(r"//[^\n]*", "", text)                       # line comments
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)           # block comments
    text = re.sub(r'"(?:\\.|[^"\\])*"', '""', text)             # string literals
    return re.sub(r"'(?:\\.|[^'\\])'", "''", text)              # char literals (lifetimes stay, they carry no brackets)


def test_patched_rust_files_are_balanced():
    """No Rust toolchain here: at least the shim's Rust files and the src/hip.rs the patch creates (rebuilt from its `+`
    lines) must keep their brackets balanced outside strings and comments (a truncated hunk or a lost brace is the kind
    of damage a hand-maintained patch suffers)."""
    (hip,) = _patch_hunks()["src/hip.rs"]
    texts = {"src/hip.rs (from the patch)": "\n".join(b[1:] for b in hip[4]) + "\n"}
    assert texts["src/hip.rs (from the patch)"].count("\n") == hip[3]
    for f in ("lib.rs", "ffi.rs", "layout.rs"):
        texts["shim/bellman-hip/src/" + f] = open(os.path.join(ROOT, "shim", "bellman-hip", "src", f)).read()
    for name, text in texts.items():
        text = _strip_rust(text)
        for o, c in ("{}", "()", "[]"):
            assert text.count(o) == text.count(c), (name, o, text.count(o), text.count(c))


def test_ffi_rs_is_generated_from_the_header():
    import gen_rust_ffi as g
    from bellman_amd import _abi, _lib

    assert open(g.OUT).read() == g.render(_abi.PRODUCT), "run python tools/gen_rust_ffi.py"
    names = [f.name for f in _abi.PRODUCT.functions]
    assert len(names) == len(set(names)) and "bh_msm_async" in names and "bh_fft_fr" in names
    assert not [n for n in names if n.startswith("bh_test_")]
    # every entry point the library exports through the product header is bound, and nothing else
    rs = open(g.OUT).read()
    assert re.findall(r"pub fn (\w+)\(", rs) == names
    assert set(names) == {s for s in _lib.EXPORTS if not s.startswith("bh_test_")}
    # every opaque handle and struct of the header, under the CamelCase of its C name
    assert g.rust_name("bh_ctx_info_t") == "BhCtxInfo" and g.rust_name("bh_r1cs_solver") == "BhR1csSolver"
    assert re.findall(r"pub struct (\w+) \{", rs) == [g.rust_name(n) for n in _abi.PRODUCT.opaque + list(_abi.PRODUCT.structs)]


def test_ffi_constants_match_the_header():
    """every #define BH_* of the header is a constant of ffi.rs with the header's value (decimal or hex), and ffi.rs holds
    no other; unsuffixed literals are c_int, `u` ones u32, *_BYTES sizes usize"""
    import gen_rust_ffi as g
    from bellman_amd import _abi

    hdr = _abi.PRODUCT.constants
    found = re.findall(r"pub const (\w+): (\w+) = (-?(?:0[xX][0-9a-fA-F]+|\d+));", open(g.OUT).read())
    assert len(found) == len(re.findall(r"pub const ", open(g.OUT).read())), "a constant of ffi.rs is not an integer literal"
    assert [name for name, _, _ in found] == list(hdr)
    for name, rtype, val in found:
        assert int(val, 0) == hdr[name].value, name
        assert rtype == ("usize" if name.endswith("_BYTES") else "u32" if hdr[name].unsigned else "c_int"), name
    # ... against the text of the header itself, read without the parser
    text = open(_abi.PRODUCT_HEADER).read()
    plain = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(BH_\w+)\s+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?\)?", text)}
    assert plain == {name: int(val, 0) for name, _, val in found}
    assert plain["BH_ERR_NO_DEVICE"] == -3 and plain["BH_R1CS_SATISFIED"] == 0xFFFFFFFF and plain["BH_MSM_SUMS_BYTES"] == 960


def test_ffi_signatures_spot_checks():
    rs = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")).read()
    assert ("pub fn bh_bases_register(ctx: *mut BhCtx, group: c_int, host_points: *const c_void, n: usize, stride: usize, "
            "inf_offset: c_long, out: *mut *mut BhBases) -> c_int;") in rs
    assert "pub fn bh_msm_wait(job: *mut BhMsmJob, out_affine: *mut c_void) -> c_int;" in rs
    assert "pub fn bh_fft_fr(ctx: *mut BhCtx, data_host: *mut c_void, log_n: u32, mode: c_int) -> c_int;" in rs
    assert "pub fn bh_point_add(group: c_int, r: *mut c_void, a: *const c_void, b: *const c_void, n: usize);" in rs
    # the wrapper only calls functions that exist
    lib_rs = open(os.path.join(ROOT, "shim", "bellman-hip", "src", "lib.rs")).read()
    for fn in set(re.findall(r"ffi::(bh_\w+)\(", lib_rs)):
        assert "pub fn %s(" % fn in rs, fn

