"""The word program the gadgets record (bellman_amd/gadgets/recorder.py) and its host side (csrc/word_program.hpp through
bh_test_word_program), without a GPU: for Sha256Preimage at 55 and 56 bytes and for the one-op circuits of
tests/models/word_circuits.py the host interpreter's witness equals WitnessAssignment synthesis with the same external words,
byte for byte; every refusal of the validator is provoked once and names the right index; recording changes nothing in the
circuit and tags every variable."""
import numpy as np
import pytest

from bellman_amd import gadgets as g
from bellman_amd.gadgets import recorder as rc
from bellman_amd.groth16 import ShapeAssembly, fr_to_mont_array
from tests.models import word_circuits as wc


def _same_as_synthesis(shape, circuit_with, row):
    ins, aux = shape.interpret(row)
    hi, ha = g.synthesize(circuit_with(row))
    assert ins.tobytes() == fr_to_mont_array(hi).tobytes()
    assert aux.tobytes() == fr_to_mont_array(ha).tobytes()


@pytest.mark.parametrize("n", [55, 56])
def test_sha256_preimage_interpreter_equals_synthesis(n):
    c = g.Sha256Preimage(n)
    shape = g.capture(c)
    assert not shape.untagged and shape.n_ext == 14 and len(shape.supplied) == 8 * n
    shape.check_program()
    plain = ShapeAssembly.capture(c)   # recording changes nothing in the circuit
    assert (plain.num_inputs, plain.num_aux) == (shape.num_inputs, shape.num_aux) and plain.rows == shape.cs.rows
    for m in (bytes(n), b"\xff" * n, bytes((i * 29 + 3) & 0xFF for i in range(n))):
        row = c.ext_from_messages([m])[0]
        ins, aux = shape.interpret(row)
        hi, ha = g.synthesize(c.with_message(m))
        assert ins.tobytes() == fr_to_mont_array(hi).tobytes() and aux.tobytes() == fr_to_mont_array(ha).tobytes()
        assert hi[1:] == c.public_inputs(m)
    # one block at 55 bytes: 48 schedule words, a and e of rounds 1 .. 63, h0 .. h7.  Two at 56: the second block is padding
    # alone, so its schedule is constant (no ADD), but its compression starts from a non-constant state
    adds = int((shape.program["instrs"][:, 0] == rc.ADD).sum())
    assert adds == len(shape.hints) and adds == (48 + 2 * 63 + 8) + (0 if n == 55 else 2 * 63 + 8)
    if n == 55:   # the last message byte shares its word with the padding's leading 1: a PACK
        assert int((shape.program["instrs"][:, 0] == rc.PACK).sum()) == 1


def test_double_sha256_records_the_second_hash_from_the_first_digest():
    c = g.Sha256Preimage(32, double=True)
    shape = g.capture(c)
    assert not shape.untagged
    m = bytes(range(100, 132))
    _same_as_synthesis(shape, lambda row: c.with_message(m), c.ext_from_messages([m])[0])
    assert int((shape.program["instrs"][:, 0] == rc.PACK).sum()) == 0   # digest words are aligned images of the sums


@pytest.mark.parametrize("kind", wc.KINDS)
def test_one_op_circuits_interpreter_equals_synthesis(kind):
    c = wc.OneOp(kind)
    shape = g.capture(c)
    assert not shape.untagged and shape.n_ext == c.n_ext and 64 <= shape.num_aux <= 1200
    shape.check_program()
    ops = set(int(x) for x in shape.program["instrs"][:, 0])
    want = {"xor": rc.XOR, "rotr_xor": rc.ROTR, "shr_xor": rc.SHR, "ch": rc.CH, "maj": rc.MAJ, "add2": rc.ADD, "add5": rc.ADD,
            "add10": rc.ADD, "pack": rc.PACK}
    if kind in want:
        assert want[kind] in ops
    if kind == "maj":
        assert rc.AND in ops
    if kind == "packed_input":
        assert [int(x) for x in shape.program["packed"][:, 2]] == [254, 2]
    for row in wc.ext_rows(kind, 12):
        _same_as_synthesis(shape, c.with_ext, row)


def test_no_recorder_records_nothing_and_untagged_booleans_stay_untagged():
    cs = ShapeAssembly()
    cs.alloc_input(lambda: 1)
    a = g.UInt32.alloc(cs, None)
    assert a.bits[0].tag() is None and a.xor(cs, a.rotr(3)).bits[0].tag() is None

    def circuit(cs):   # a Boolean operation outside UInt32, without a tag
        x = g.UInt32.alloc(cs, None)
        g.Boolean.and_(cs, x.bits[0], x.bits[1])
    shape = g.capture(circuit)
    assert shape.untagged == [shape.num_inputs + 32]
    with pytest.raises(g.WordProgramError) as e:
        shape.check_program()
    assert (e.value.code, e.value.index) == (g.BAD_UNCOVERED, 33)


# ---- the validator's refusals ----------------------------------------------------------------------------------------------
def _base():
    """1 input (ONE), 3 aux, 1 external word; word 1 = CONST, word 2 = XOR(0, 1), word 3 = ADD(0, 1), word 4 = PACK"""
    bits = [(0, i) for i in range(32)] + [(2, 0), (2, 1 | (1 << 8))]
    return dict(n_ext=1,
                instrs=np.array([(rc.CONST, 5, 0, 0), (rc.XOR, 0, 1, 0), (rc.ADD, 0, 2, 0), (rc.PACK, 0, 0, 0)], dtype=np.uint32),
                pool=np.array([0, 1], dtype=np.uint32), bits=np.array(bits, dtype=np.uint32),
                bit_vars=np.array([(1, 2, 0), (2, 3, 32)], dtype=np.uint32), packed=np.array([(3, 32, 2)], dtype=np.uint32))


def _refused(program, n_inputs=1, n_aux=3):
    with pytest.raises(g.WordProgramError) as e:
        g.check_program(n_inputs, n_aux, program)
    return e.value.code, e.value.index


def test_validator_accepts_the_base_program_and_interprets_it():
    p = _base()
    g.check_program(1, 3, p)
    ins, aux, words = g.interpret(1, 3, p, [0x80000003])
    assert list(words) == [0x80000003, 5, 0x80000006, 0x80000008, 0x80000003]
    one = fr_to_mont_array([1])[0]
    assert ins[0].tobytes() == one.tobytes()
    # aux 0 = bit 0 of word 2 = 0; aux 1 = bit 32 of the sum (the carry) = 0; aux 2 = bit0(w2) + 2 * !bit1(w2) = 0 + 0
    assert not aux.any()
    ins, aux, words = g.interpret(1, 3, p, [0xFFFFFFFC])
    assert int(words[3]) == 0xFFFFFFFC + 5 and aux.tobytes() == fr_to_mont_array([1, 1, 3]).tobytes()


def test_validator_refusals_name_the_index():
    p = _base()
    p["instrs"][1] = (rc.XOR, 0, 2, 0)           # reads its own word
    assert _refused(p) == (g.BAD_SOURCE, 1)
    p = _base()
    p["instrs"][1] = (rc.ROTR, 3, 1, 0)          # reads a later word
    assert _refused(p) == (g.BAD_SOURCE, 1)
    p = _base()
    p["pool"][1] = 3                             # an ADD source that is its own destination
    assert _refused(p) == (g.BAD_SOURCE, 2)
    p = _base()
    p["bits"][7] = (4, 0)                        # a PACK source that is its own destination
    assert _refused(p) == (g.BAD_SOURCE, 3)
    p = _base()
    p["bits"][31] = (0, 64)
    assert _refused(p) == (g.BAD_BIT, 3)
    for count in (1, 11):
        p = _base()
        p["pool"] = np.zeros(16, dtype=np.uint32)
        p["instrs"][2] = (rc.ADD, 0, count, 0)
        assert _refused(p) == (g.BAD_ADD_ARITY, 2)
    p = _base()
    p["instrs"][2] = (rc.ADD, 1, 2, 0)           # leaves its pool
    assert _refused(p) == (g.BAD_OP, 2)
    p = _base()
    p["instrs"][0] = (0, 0, 0, 0)
    assert _refused(p) == (g.BAD_OP, 0)
    p = _base()
    p["instrs"][1] = (rc.SHR, 0, 32, 0)
    assert _refused(p) == (g.BAD_OP, 1)
    p = _base()
    p["bits"] = np.array([(0, i % 32) for i in range(32 + 255)], dtype=np.uint32)
    p["packed"] = np.array([(3, 32, 255)], dtype=np.uint32)
    assert _refused(p) == (g.BAD_PACKED_BITS, 3)
    p["packed"] = np.array([(3, 32, 254)], dtype=np.uint32)
    g.check_program(1, 3, p)
    p = _base()
    p["bit_vars"][1] = (4, 3, 0)
    assert _refused(p) == (g.BAD_VAR_RANGE, 1)
    p = _base()
    p["packed"][0] = (9, 32, 2)
    assert _refused(p) == (g.BAD_VAR_RANGE, 2)   # bit records first: the packed record is record 2
    p = _base()
    p["bit_vars"][0] = (1, 5, 0)                 # word 5 does not exist
    assert _refused(p) == (g.BAD_VAR_SOURCE, 1)
    p = _base()
    p["bit_vars"][1] = (2, 3, 64)
    assert _refused(p) == (g.BAD_VAR_SOURCE, 2)
    p = _base()
    p["bit_vars"] = p["bit_vars"][1:]            # variables 1 is uncovered
    assert _refused(p) == (g.BAD_UNCOVERED, 1)
    p = _base()
    assert _refused(p, n_aux=5) == (g.BAD_UNCOVERED, 4)   # the lowest of 4 and 5
    p = _base()
    p["bit_vars"] = np.concatenate([p["bit_vars"], np.array([(3, 0, 0)], dtype=np.uint32)])   # also packed
    assert _refused(p) == (g.BAD_COVERED_TWICE, 3)
    p = _base()
    p["bit_vars"] = np.concatenate([p["bit_vars"], np.array([(0, 0, 0)], dtype=np.uint32)])   # ONE
    assert _refused(p) == (g.BAD_COVERED_TWICE, 0)


def test_header_and_python_constants_agree():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bellman_hip.h")).read()
    defs = dict(re.findall(r"#define\s+(BH_WORD_\w+)\s+(\d+)", hdr))
    for name in ("CONST", "ROTR", "SHR", "XOR", "AND", "CH", "MAJ", "ADD", "PACK"):
        assert int(defs["BH_WORD_" + name]) == getattr(rc, name)
    for name in ("SOURCE", "BIT", "ADD_ARITY", "OP", "VAR_SOURCE", "PACKED_BITS", "VAR_RANGE", "UNCOVERED", "COVERED_TWICE"):
        assert int(defs["BH_WORD_BAD_" + name]) == getattr(g, "BAD_" + name)


def test_validator_and_interpreter_under_host_sanitizers(tmp_path):
    """csrc/word_program.hpp in a stand-alone program of its own (tests/cpp/word_program_san.cpp, a toy field), built with
    AddressSanitizer and UndefinedBehaviorSanitizer and run as a process: nothing loaded into Python is involved"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "word_program_san.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "cpp", "word_program_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "word_program ok", (r.returncode, r.stdout, r.stderr)
