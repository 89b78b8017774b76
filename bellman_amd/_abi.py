"""The C ABI as include/bellman_hip.h and include/bellman_hip_test.h state it, parsed once: the functions, opaque
handles, structs and integer constants of the two headers, and from them the ctypes types of every signature, one
ctypes structure class per header struct and the constants by name (`C.BH_OK`).  _lib.py binds the libraries from this,
tools/gen_rust_ffi.py renders the Rust declarations from it: the headers are the only statement of the boundary.

Standard library only, no HIP call.  The parser is strict: a type it does not know, a `bh_*(` it cannot read as a
declaration, a struct it cannot close or a `#define BH_*` that is no integer literal raises AbiError naming the symbol."""

import collections
import ctypes
import os
import re
import types

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
PRODUCT_HEADER = os.path.join(INCLUDE_DIR, "bellman_hip.h")
TEST_HEADER = os.path.join(INCLUDE_DIR, "bellman_hip_test.h")


class AbiError(ValueError):
    pass


# name, C return type, [(parameter name, C type)]; C types are normalised text: "const uint64_t *", "bh_bases **"
Function = collections.namedtuple("Function", "name ret params")
# value, whether the literal carries a `u` suffix, and the literal as written without it (rendered as is: hex stays hex)
Constant = collections.namedtuple("Constant", "value unsigned text")
# functions: [Function]; opaque: [name]; structs: {name: [(field, C type)]}; constants: {name: Constant} - in header order
Header = collections.namedtuple("Header", "functions opaque structs constants")

SCALARS = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "long": ctypes.c_long,
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
    "float": ctypes.c_float, "double": ctypes.c_double, "unsigned char": ctypes.c_ubyte,
}
_INT = r"(?:0[xX][0-9a-fA-F]+|\d+)"
_POINTEES = ("void", "char")   # known base types that appear behind a pointer only


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def split_type(ctype):
    """'const bh_ctx *const *' -> (True, 'bh_ctx', [True, False]): the base's const, the base type, and per pointer
    level whether `const` follows its `*`; None when the text is no type of this shape"""
    m = re.match(r"^(const\s+)?([A-Za-z_][\w ]*?)\s*((?:\*\s*(?:const\s*)?)*)$", ctype.strip())
    if not m:
        return None
    return bool(m.group(1)), " ".join(m.group(2).split()), [bool(q) for q in re.findall(r"\*\s*(const)?", m.group(3))]


def _checked_type(ctype, known, symbol):
    parts = split_type(ctype)
    if parts is None or parts[1] not in known:
        raise AbiError("%s: unknown C type %r" % (symbol, " ".join(ctype.split())))
    if parts[1] in _POINTEES and not parts[2] and ctype.strip() != "void":
        raise AbiError("%s: %r by value" % (symbol, ctype.strip()))
    return " ".join(ctype.split())


def _line_of(text, pos):
    return text.count("\n", 0, pos) + 1


def parse(text, known=()):
    """One header's text -> Header.  `known`: type names declared by a header this one includes."""
    text = strip_comments(text)
    constants = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(BH_\w+)(.*)$", text, flags=re.M):
        name, rest = m.group(1), m.group(2)
        # a function-like macro has its parenthesis directly behind the name
        lit = None if rest[:1] == "(" else re.match(r"^(?:\((-?%s)([uU]?)\)|(-?%s)([uU]?))$" % (_INT, _INT), rest.strip())
        if not lit:
            raise AbiError("%s: #define is not an integer literal: %r" % (name, rest.strip()))
        digits, suffix = lit.group(1) or lit.group(3), lit.group(2) or lit.group(4)
        constants[name] = Constant(int(digits, 0), bool(suffix), digits)
    text = re.sub(r"^[ \t]*#.*$", lambda m: " " * len(m.group(0)), text, flags=re.M)   # same length: line numbers hold

    known = set(SCALARS) | set(_POINTEES) | set(known)
    functions, opaque, structs = [], [], {}
    pos, extern_c = 0, 0
    while True:
        pos = re.compile(r"\s*").match(text, pos).end()
        if pos == len(text):
            break
        m = re.compile(r'extern\s+"C"\s*\{').match(text, pos)
        if m:
            extern_c += 1
            pos = m.end()
            continue
        if text[pos] == "}" and extern_c:
            extern_c -= 1
            pos += 1
            continue
        m = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;").match(text, pos)
        if m:
            if m.group(1) != m.group(2):
                raise AbiError("%s: opaque typedef of another tag %r" % (m.group(2), m.group(1)))
            opaque.append(m.group(2))
            known.add(m.group(2))
            pos = m.end()
            continue
        m = re.compile(r"typedef\s+struct\s*(\w*)\s*\{").match(text, pos)
        if m:
            body = re.compile(r"([^{}]*)\}\s*(\w+)\s*;").match(text, m.end())
            if not body:
                raise AbiError("struct %s (line %d): no closing `} name;`" % (m.group(1) or "<anonymous>", _line_of(text, pos)))
            name = body.group(2)
            fields = []
            for decl in body.group(1).split(";"):
                if not decl.strip():
                    continue
                d = re.match(r"^(.*?)(\w+(?:\s*,\s*\w+)*)$", decl.strip(), flags=re.S)
                if not d or not d.group(1).strip():
                    raise AbiError("struct %s: cannot read the field %r" % (name, " ".join(decl.split())))
                ctype = _checked_type(d.group(1), known, "struct " + name)
                fields += [(f.strip(), ctype) for f in d.group(2).split(",")]
            structs[name] = fields
            known.add(name)
            pos = body.end()
            continue
        end = text.find(";", pos)
        stmt = text[pos:end if end >= 0 else len(text)]
        symbol = re.search(r"\bbh_\w+", stmt)
        symbol = symbol.group(0) if symbol else "line %d" % _line_of(text, pos)
        m = re.match(r"^([A-Za-z_][\w\s\*]*?)\b(bh_\w+)\s*\(([^()]*)\)\s*$", stmt, flags=re.S)
        if end < 0 or not m:
            raise AbiError("%s: cannot read %r as a function declaration" % (symbol, " ".join(stmt.split())[:120]))
        name, args = m.group(2), " ".join(m.group(3).split())
        ret = _checked_type(m.group(1), known, name)
        params = []
        if args != "void":
            for a in args.split(","):
                arr = re.match(r"^(.*?)(\w+)\s*\[\d*\]$", a.strip())
                if arr:   # an array parameter decays to a pointer
                    ctype, pname = arr.group(1) + "*", arr.group(2)
                else:
                    p = re.match(r"^(.*?)(\w+)$", a.strip())
                    if not p or not p.group(1).strip():
                        raise AbiError("%s: cannot read the parameter %r" % (name, a.strip()))
                    ctype, pname = p.group(1), p.group(2)
                if ctype.strip() == "void":
                    raise AbiError("%s: parameter %r of type void" % (name, pname))
                params.append((pname, _checked_type(ctype, known, name)))
        functions.append(Function(name, ret, params))
        pos = end + 1
    if extern_c:
        raise AbiError('extern "C" { is not closed')
    return Header(functions, opaque, structs, constants)


def _read(path):
    if not os.path.exists(path):
        raise AbiError("%s not found: the bindings of bellman_amd are derived from the C headers" % path)
    with open(path) as f:
        return f.read()


def _parse_headers():
    product = parse(_read(PRODUCT_HEADER))
    test = parse(_read(TEST_HEADER), known=product.opaque + list(product.structs))   # it includes the product header
    return product, test


PRODUCT, TEST = _parse_headers()
# every BH_* constant of the two headers by name
C = types.SimpleNamespace(**{k: c.value for h in (PRODUCT, TEST) for k, c in h.constants.items()})


def ctype_of(ctype):
    """The ctypes type of a parameter, field or return type: every pointer is c_void_p (`const char *` as a return type
    is c_char_p, see restype_of), scalars are exact, a struct by value is its derived class; None for void."""
    _, base, levels = split_type(ctype)
    if levels:
        return ctypes.c_void_p
    if base == "void":
        return None
    return SCALARS[base] if base in SCALARS else STRUCTS[base]


def restype_of(ctype):
    return ctypes.c_char_p if ctype == "const char *" else ctype_of(ctype)


# the ctypes class of every header struct, by its C name: the header's field names, in the header's order
STRUCTS = {}
for _h in (PRODUCT, TEST):
    for _name, _fields in _h.structs.items():
        STRUCTS[_name] = type(_name, (ctypes.Structure,), {"_fields_": [(f, ctype_of(t)) for f, t in _fields]})
