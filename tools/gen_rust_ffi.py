"""Generates shim/bellman-hip/src/ffi.rs - the Rust `extern "C"` block - from include/bellman_hip.h so the
two cannot drift (tests/test_shim_cpu.py regenerates and compares).  No Rust toolchain exists in this image:
the output is checked structurally here and compiled by whoever applies the shim.

Usage: python tools/gen_rust_ffi.py [--check]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bellman_hip.h")
OUT = os.path.join(ROOT, "shim", "bellman-hip", "src", "ffi.rs")

OPAQUE = {"bh_ctx": "BhCtx", "bh_bases": "BhBases", "bh_msm_job": "BhMsmJob", "bh_params": "BhParams", "bh_r1cs": "BhR1cs",
          "bh_scalars": "BhScalars", "bh_msm_sharded_job": "BhMsmShardedJob", "bh_proof_job": "BhProofJob",
          "bh_pvk": "BhPvk", "bh_pvk_set": "BhPvkSet", "bh_msm_many_job": "BhMsmManyJob", "bh_r1cs_solver": "BhR1csSolver",
          "bh_word_witness": "BhWordWitness"}
STRUCTS = {"bh_csr": "BhCsr", "bh_msm_opts": "BhMsmOpts", "bh_ctx_info_t": "BhCtxInfo",
           "bh_powers_of_tau": "BhPowersOfTau", "bh_ptau_report": "BhPtauReport",
           "bh_params_step_report": "BhParamsStepReport", "bh_witness_hint": "BhWitnessHint", "bh_solver_desc": "BhSolverDesc",
           "bh_word_instr": "BhWordInstr", "bh_word_bit": "BhWordBit", "bh_word_var": "BhWordVar", "bh_word_packed": "BhWordPacked",
           "bh_word_witness_desc": "BhWordWitnessDesc"}
SCALAR = {
    "int": "c_int", "unsigned": "c_uint", "unsigned int": "c_uint", "long": "c_long", "uint32_t": "u32", "uint64_t": "u64",
    "int32_t": "i32", "size_t": "usize", "float": "f32", "double": "f64", "char": "c_char", "void": "c_void",
}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def c_type_to_rust(ctype):
    """'const uint64_t *' -> '*const u64' ; 'bh_bases **' -> '*mut *mut BhBases'"""
    t = ctype.strip()
    # base type (with its own leading const), then one `*` per pointer level, each optionally followed by `const`
    # ("bh_ctx *const *": pointer to const pointer to BhCtx -> *const *mut BhCtx)
    m = re.match(r"^(const\s+)?([A-Za-z_][\w ]*?)\s*((?:\*\s*(?:const\s*)?)*)$", t)
    if not m:
        raise ValueError("unknown C type %r" % ctype)
    const, base = bool(m.group(1)), " ".join(m.group(2).split())
    levels = re.findall(r"\*\s*(const)?", m.group(3))
    if base in OPAQUE:
        r = OPAQUE[base]
    elif base in STRUCTS:
        r = STRUCTS[base]
    elif base in SCALAR:
        r = SCALAR[base]
    else:
        raise ValueError("unknown C type %r" % ctype)
    if not levels:
        return r
    # the pointee of level k is const when the qualifier to its left says so: the base's `const` for the innermost
    # pointer, the `const` after the previous `*` for the others; an unqualified outer pointer is an out-parameter
    quals = [const] + [bool(q) for q in levels[:-1]]
    out = r
    for q in quals:
        out = ("*const " if q else "*mut ") + out
    return out


def parse_decls(text):
    text = strip_comments(text)
    text = re.sub(r"typedef struct \{.*?\} \w+;", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern "C" \{', " ", text)
    decls = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(bh_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        if ret.startswith("typedef"):
            continue
        params = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                arr = re.match(r"(.*?)(\w+)\s*\[\d*\]$", a)
                if arr:   # array parameter decays to a pointer
                    ctype, pname = arr.group(1) + "*", arr.group(2)
                else:
                    mm = re.match(r"(.*?)(\w+)$", a)
                    ctype, pname = mm.group(1), mm.group(2)
                params.append((pname, c_type_to_rust(ctype)))
        rret = None if ret == "void" else c_type_to_rust(ret)
        decls.append((name, params, rret))
    return decls


RUST_KEYWORDS = {"type", "in", "ref", "box", "move", "fn", "as", "loop", "match", "where", "use", "mod"}


def render(decls):
    lines = [
        "//! `extern \"C\"` declarations of libbellman_hip - GENERATED from include/bellman_hip.h by",
        "//! tools/gen_rust_ffi.py; do not edit.  One item per C entry point, same order, same argument names.",
        "#![allow(non_camel_case_types, dead_code)]",
        "use std::os::raw::{c_char, c_int, c_long, c_uint, c_void};",
        "",
    ]
    for c, r in OPAQUE.items():
        lines += ["/// opaque `%s`" % c, "#[repr(C)]", "pub struct %s {" % r, "    _private: [u8; 0],", "}"]
    lines += [
        "/// `bh_csr`: one constraint matrix in CSR form (include/bellman_hip.h)",
        "#[repr(C)]", "#[derive(Clone, Copy)]",
        "pub struct BhCsr {", "    pub row_ptr: *const u32,", "    pub var: *const u32,", "    pub coeff: *const u32,", "}",
        "/// `bh_msm_opts`: per-job plan overrides; all-zero = tuned defaults",
        "#[repr(C)]", "#[derive(Clone, Copy, Default)]",
        "pub struct BhMsmOpts {", "    pub window_bits: u32,", "    pub chunk: u32,", "    pub flags: u32,", "}",
        "/// `bh_ctx_info_t`: what bh_ctx_info reports about a context",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhCtxInfo {", "    pub device: i32,", "    pub num_cus: u32,", "    pub hbm_bytes: u64,",
        "    pub hw_queues_requested: u32,", "    pub hw_queues_set_before_hip_init: u32,", "    pub max_jobs_in_flight: u32,",
        "    pub jobs_in_flight: u32,", "    pub pool_bytes_held: u64,", "    pub pool_bytes_idle: u64,", "    pub table_bytes: u64,",
        "    pub table_budget: u64,", "    pub fft_table_bytes: u64,", "    pub fft_table_budget: u64,", "}",
        "/// `bh_powers_of_tau`: a powers-of-tau transcript as device-resident handles plus [beta]G2 on the host",
        "#[repr(C)]", "#[derive(Clone, Copy)]",
        "pub struct BhPowersOfTau {", "    pub tau_g1: *const BhBases,", "    pub tau_g2: *const BhBases,",
        "    pub alpha_tau_g1: *const BhBases,", "    pub beta_tau_g1: *const BhBases,", "    pub beta_g2: *const c_void,", "}",
        "/// `bh_ptau_report`: what bh_powers_of_tau_verify found (the BH_PTAU_FAILED_* bits; the first bad point)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhPtauReport {", "    pub failed: u32,", "    pub bad_vector: u32,", "    pub bad_index: usize,", "}",
        "/// `bh_params_step_report`: what bh_groth16_params_verify_step found (the BH_STEP_FAILED_* bits; the first position)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhParamsStepReport {", "    pub failed: u32,", "    pub bad_vector: u32,", "    pub bad_index: usize,", "}",
        "/// `bh_witness_hint`: one hint of a witness solver (kind = BH_HINT_*; terms and outputs as ranges of the pools)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhWitnessHint {", "    pub kind: u32,", "    pub lc_begin: u32,", "    pub lc_end: u32,", "    pub out_begin: u32,",
        "    pub out_end: u32,", "    pub shift: u32,", "}",
        "/// `bh_solver_desc`: what bh_r1cs_solver_create takes besides the circuit: supplied variables and hints",
        "#[repr(C)]", "#[derive(Clone, Copy)]",
        "pub struct BhSolverDesc {", "    pub supplied: *const u32,", "    pub n_supplied: usize,", "    pub hints: *const BhWitnessHint,",
        "    pub n_hints: usize,", "    pub lc_var: *const u32,", "    pub lc_coeff: *const u32,", "    pub out_var: *const u32,",
        "    pub hint_coeffs: *const c_void,", "    pub n_hint_coeffs: usize,", "}",
        "/// `bh_word_instr`: one instruction of a word program (op = BH_WORD_*)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhWordInstr {", "    pub op: u32,", "    pub a: u32,", "    pub b: u32,", "    pub c: u32,", "}",
        "/// `bh_word_bit`: a bit source (bit | neg << 8 of a trace word)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhWordBit {", "    pub word: u32,", "    pub bit_neg: u32,", "}",
        "/// `bh_word_var`: the record of a bit variable",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhWordVar {", "    pub var: u32,", "    pub word: u32,", "    pub bit_neg: u32,", "}",
        "/// `bh_word_packed`: the record of a packed variable (a range of bit sources)",
        "#[repr(C)]", "#[derive(Clone, Copy, Default, Debug)]",
        "pub struct BhWordPacked {", "    pub var: u32,", "    pub bits_begin: u32,", "    pub n_bits: u32,", "}",
        "/// `bh_word_witness_desc`: what bh_word_witness_create takes: the program and the variable records",
        "#[repr(C)]", "#[derive(Clone, Copy)]",
        "pub struct BhWordWitnessDesc {", "    pub n_inputs: usize,", "    pub n_aux: usize,", "    pub n_ext: usize,",
        "    pub instrs: *const BhWordInstr,", "    pub n_instrs: usize,", "    pub pool: *const u32,", "    pub n_pool: usize,",
        "    pub bits: *const BhWordBit,", "    pub n_bits: usize,", "    pub vars: *const BhWordVar,", "    pub n_vars: usize,",
        "    pub packed: *const BhWordPacked,", "    pub n_packed: usize,", "}",
        "",
    ]
    consts = [("BH_OK", 0), ("BH_ERR_UNEXPECTED_IDENTITY", 1), ("BH_ERR_UNEXPECTED_EOF", 2), ("BH_ERR_DEGREE_TOO_LARGE", 3),
              ("BH_ERR_UNCONSTRAINED_VARIABLE", 5), ("BH_ERR_INVALID_POINT", 6), ("BH_ERR_POINT_AT_INFINITY", 7),
              ("BH_ERR_INVALID_TRANSCRIPT", 10), ("BH_ERR_HIP", -1), ("BH_ERR_INVALID_ARG", -2), ("BH_ERR_NO_DEVICE", -3), ("BH_SCALARS_CANONICAL", 0),
              ("BH_SCALARS_MONT", 1), ("BH_G1", 1), ("BH_G2", 2), ("BH_FFT", 0), ("BH_IFFT", 1), ("BH_COSET_FFT", 2),
              ("BH_ICOSET_FFT", 3)]
    for k, v in consts:
        lines.append("pub const %s: c_int = %d;" % (k, v))
    lines += ["pub const BH_POINTS_CHECKED: c_uint = 1;", "pub const BH_POINTS_FORBID_IDENTITY: c_uint = 2;",
              "pub const BH_PTAU_VALIDATE_POINTS: c_uint = 1;", "pub const BH_STEP_VALIDATE_POINTS: c_uint = 1;",
              "pub const BH_HINT_BITS: u32 = 1;", "pub const BH_HINT_INV_OR_ZERO: u32 = 2;"]
    lines += ["pub const BH_WORD_%s: u32 = %d;" % (k, i + 1) for i, k in enumerate(
        ("CONST", "ROTR", "SHR", "XOR", "AND", "CH", "MAJ", "ADD", "PACK"))]
    lines += ["pub const BH_WORD_BAD_%s: u32 = %d;" % (k, i + 1) for i, k in enumerate(
        ("SOURCE", "BIT", "ADD_ARITY", "OP", "VAR_SOURCE", "PACKED_BITS", "VAR_RANGE", "UNCOVERED", "COVERED_TWICE"))]
    lines += ["pub const %s: u32 = 0x%02x;" % (k, v) for k, v in
              (("BH_PTAU_FAILED_HEAD", 1), ("BH_PTAU_FAILED_TAU_G1_G2", 2), ("BH_PTAU_FAILED_TAU_G1", 4), ("BH_PTAU_FAILED_TAU_G2", 8),
               ("BH_PTAU_FAILED_ALPHA", 16), ("BH_PTAU_FAILED_BETA", 32), ("BH_PTAU_FAILED_BETA_G2", 64), ("BH_PTAU_FAILED_POINTS", 128))]
    lines += ["pub const %s: u32 = 0x%03x;" % (k, 1 << i) for i, k in enumerate(
        ("BH_STEP_FAILED_SHAPE", "BH_STEP_FAILED_HEAD", "BH_STEP_FAILED_KEY", "BH_STEP_FAILED_A", "BH_STEP_FAILED_B_G1",
         "BH_STEP_FAILED_B_G2", "BH_STEP_FAILED_DELTA", "BH_STEP_FAILED_H", "BH_STEP_FAILED_L", "BH_STEP_FAILED_POINTS"))]
    lines += ["pub const BH_MSM_SUMS_BYTES: usize = 960;", "", "#[link(name = \"bellman_hip\")]", "extern \"C\" {"]
    for name, params, ret in decls:
        ps = ", ".join("%s: %s" % (("r#" + p) if p in RUST_KEYWORDS else p, t) for p, t in params)
        lines.append("    pub fn %s(%s)%s;" % (name, ps, (" -> " + ret) if ret else ""))
    lines += ["}", ""]
    return "\n".join(lines)


def header_constants():
    text = open(HEADER).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"#define\s+(BH_\w+)\s+\(?(-?\d+)u?\)?", text)}


def main():
    decls = parse_decls(open(HEADER).read())
    out = render(decls)
    if "--check" in sys.argv:
        cur = open(OUT).read()
        if cur != out:
            print("shim/bellman-hip/src/ffi.rs is stale: run python tools/gen_rust_ffi.py")
            sys.exit(1)
        print("ffi.rs matches include/bellman_hip.h (%d entry points)" % len(decls))
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write(out)
    print("wrote %s (%d entry points)" % (OUT, len(decls)))


if __name__ == "__main__":
    main()
