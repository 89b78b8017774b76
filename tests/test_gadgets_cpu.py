"""The gadget layer of SHA-256 (bellman_amd/gadgets: boolean, uint32, multieq, sha256, multipack - the reference's
src/gadgets restated) without a GPU: the reference's own pins (sha256.rs test_blank_hash, test_full_block,
test_against_vectors), every case row of the Boolean operations against the truth table with the allocation count the
reference's case table implies, addmany at its operand-count and carry edges, and MultiEq's emission points.  Satisfaction
is judged by evaluating a * b = c of every constraint in Python integers (ProvingAssignment's evaluations)."""
import hashlib
import itertools

import pytest

from bellman_amd import gadgets as g
from bellman_amd.groth16 import ProvingAssignment, Q, ShapeAssembly
from bellman_amd.gadgets.sha256 import get_sha256_iv


def _cs():
    cs = ProvingAssignment()
    cs.alloc_input(lambda: 1)
    return cs


def _satisfied(cs):
    return all(a * b % Q == c for a, b, c in zip(cs.a, cs.b, cs.c))


def _digest_bytes(bits):
    vals = [b.get_value() for b in bits]
    assert None not in vals
    return bytes(sum(int(v) << (7 - i) for i, v in enumerate(vals[lo:lo + 8])) for lo in range(0, len(vals), 8))


def test_blank_hash():
    """sha256.rs:283-304: the all-constant block (a lone leading 1, the padding of the empty message) costs no constraint
    and gives SHA-256 of the empty string"""
    cs = _cs()
    bits = [g.Boolean.constant(False)] * 512
    bits[0] = g.Boolean.constant(True)
    out = g.sha256_compression_function(cs, bits, get_sha256_iv())
    assert len(cs.a) == 0 and len(cs.aux_assignment) == 0
    digest = _digest_bytes([b for e in out for b in e.into_bits_be()])
    assert digest.hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert all(b.is_constant() for e in out for b in e.bits)


def test_full_block():
    """sha256.rs:307-332: one compression over 512 allocated bits: num_constraints - 512 == 25840"""
    cs = ShapeAssembly()
    cs.alloc_input(lambda: 1)
    bits = [g.Boolean.Is(g.AllocatedBit.alloc(cs, None)) for _ in range(512)]
    g.sha256_compression_function(cs, bits, get_sha256_iv())
    assert len(cs.rows[0]) - 512 == 25840


# sha256.rs:335-385 test_against_vectors sweeps every length below 32 bytes and the multiples of 8 from 32 to 248 (:343); to keep
# the run short this takes every length below 32 and then 32, 55, 56, 64, 119, 120, 248 (the block edges, and the longest)
LENGTHS = list(range(32)) + [32, 55, 56, 64, 119, 120, 248]


@pytest.mark.parametrize("n", LENGTHS)
def test_against_vectors(n):
    message = bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n))
    cs = _cs()
    bits = [g.Boolean.Is(g.AllocatedBit.alloc(cs, v)) for v in g.bytes_to_bits(message)]
    out = g.sha256(cs, bits)
    assert _digest_bytes(out) == hashlib.sha256(message).digest()
    assert _satisfied(cs)
    for b, want in zip(out, g.bytes_to_bits(hashlib.sha256(message).digest())):   # as the reference: the variable itself
        if not b.is_constant():
            assert cs.aux_assignment[b.bit.variable.idx] == (int(want) if b.kind == 1 else 1 - int(want))


def test_preimage_circuit_exposes_the_digest():
    for n, double in ((3, False), (32, True)):
        c = g.Sha256Preimage(n, double)
        m = bytes(range(n))
        cs = _cs()
        c.with_message(m)(cs)
        assert _satisfied(cs) and cs.input_assignment[1:] == c.public_inputs(m) and len(cs.input_assignment) == 3
        d = hashlib.sha256(m).digest()
        assert c.digest(m) == (hashlib.sha256(d).digest() if double else d)
        assert list(c.ext_from_messages([m])[0]) == [int.from_bytes((m + b"\0\0\0")[4 * e:4 * e + 4], "big") for e in range(c.n_ext)]


# ---- the case tables of Boolean.xor / and / sha256_ch / sha256_maj -------------------------------------------------------
KINDS = ("F", "T", "Is", "Not")


def _operand(cs, kind, value):
    """-> (Boolean, its logical value): value is the logical value wanted from a non-constant operand"""
    if kind in ("F", "T"):
        return g.Boolean.constant(kind == "T"), kind == "T"
    if kind == "Is":
        return g.Boolean.Is(g.AllocatedBit.alloc(cs, value)), value
    return g.Boolean.Not(g.AllocatedBit.alloc(cs, not value)), value


def _const(k):
    return k in ("F", "T")


def _and_allocs(x, y):
    """boolean.rs:486-512: a constant operand folds, every other pair allocates one variable"""
    return 0 if _const(x) or _const(y) else 1


def _ch_allocs(a, b, c):
    """boolean.rs:533-595, case by case in the reference's order"""
    if _const(a) and _const(b) and _const(c):
        return 0
    if a == "F":
        return 0
    if b == "F":
        return _and_allocs(a, c)
    if c == "F" or c == "T":
        return _and_allocs(a, b)
    if b == "T":
        return _and_allocs(a, c)
    return 1


def _maj_allocs(a, b, c):
    """boolean.rs:640-698; the general case allocates maj and b AND c"""
    if _const(a) and _const(b) and _const(c):
        return 0
    if _const(a):
        return _and_allocs(b, c)
    if _const(b):
        return _and_allocs(a, c)
    if _const(c):
        return _and_allocs(a, b)
    return 2


OPS = {
    "xor": (2, lambda cs, a, b: g.Boolean.xor(cs, a, b), lambda a, b: a ^ b, lambda a, b: _and_allocs(a, b)),
    "and": (2, lambda cs, a, b: g.Boolean.and_(cs, a, b), lambda a, b: a & b, _and_allocs),
    "ch": (3, lambda cs, a, b, c: g.Boolean.sha256_ch(cs, a, b, c), lambda a, b, c: (a & b) ^ ((not a) & c), _ch_allocs),
    "maj": (3, lambda cs, a, b, c: g.Boolean.sha256_maj(cs, a, b, c), lambda a, b, c: (a & b) ^ (a & c) ^ (b & c), _maj_allocs),
}


@pytest.mark.parametrize("op", list(OPS))
def test_boolean_case_tables(op):
    arity, fn, truth, allocs = OPS[op]
    for kinds in itertools.product(KINDS, repeat=arity):
        free = [i for i, k in enumerate(kinds) if not _const(k)]
        for assignment in itertools.product((False, True), repeat=len(free)):
            cs = _cs()
            vals = dict(zip(free, assignment))
            operands = [_operand(cs, k, vals.get(i)) for i, k in enumerate(kinds)]
            before = len(cs.aux_assignment)
            out = fn(cs, *[o[0] for o in operands])
            want = bool(truth(*[o[1] for o in operands]))
            assert out.get_value() == want, (op, kinds, assignment)
            assert _satisfied(cs), (op, kinds, assignment)
            assert len(cs.aux_assignment) - before == allocs(*kinds), (op, kinds)
            if not out.is_constant():   # the variable behind the result holds it
                v = cs.aux_assignment[out.bit.variable.idx]
                assert v == (int(want) if out.kind == 1 else 1 - int(want))


def test_allocated_bit_gates_and_not():
    for a, b in itertools.product((False, True), repeat=2):
        cs = _cs()
        x, y = g.AllocatedBit.alloc(cs, a), g.AllocatedBit.alloc(cs, b)
        assert g.AllocatedBit.xor(cs, x, y).value == (a ^ b) and g.AllocatedBit.and_(cs, x, y).value == (a & b)
        assert g.AllocatedBit.and_not(cs, x, y).value == (a & (not b)) and g.AllocatedBit.nor(cs, x, y).value == ((not a) & (not b))
        assert _satisfied(cs) and len(cs.a) == 6
    cs2 = _cs()
    v = cs2.alloc(lambda: 2)   # not a bit: the boolean constraint must fail
    one = cs2.one()
    cs2.enforce(lambda lc: lc + one - v, lambda lc: lc + v, lambda lc: lc)
    assert not _satisfied(cs2)
    b = g.Boolean.Is(g.AllocatedBit.alloc(_cs(), True))
    assert b.not_().get_value() is False and b.not_().not_().get_value() is True and g.Boolean.constant(True).not_().const is False


# ---- addmany ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops,result_bits", [(2, 33), (5, 35), (10, 36)])
def test_addmany_operand_counts_and_carries(n_ops, result_bits):
    specials = (0, 0xFFFFFFFF, 0x80000001)
    for values in ([0] * n_ops, [0xFFFFFFFF] * n_ops, [0x80000001] * n_ops, [specials[i % 3] for i in range(n_ops)],
                   [(0x9E3779B9 * (i + 1)) & 0xFFFFFFFF for i in range(n_ops)]):
        cs = _cs()
        ops = [g.UInt32.alloc(cs, v) for v in values]
        before = len(cs.aux_assignment)
        with g.MultiEq(cs) as m:
            r = g.UInt32.addmany(m, ops)
        assert len(cs.aux_assignment) - before == result_bits and len(r.bits) == 32
        assert r.value == sum(values) & 0xFFFFFFFF and _satisfied(cs)
        total = sum(cs.aux_assignment[before + i] << i for i in range(result_bits))
        assert total == sum(values)   # the carry bits hold the full sum
        assert [b.get_value() for b in r.bits] == [bool((r.value >> i) & 1) for i in range(32)]


def test_addmany_with_constants_and_all_constant():
    cs = _cs()
    a = g.UInt32.alloc(cs, 0xFFFFFFFF)
    not_a = g.UInt32.from_bits([b.not_() for b in a.bits])
    before = len(cs.aux_assignment)
    with g.MultiEq(cs) as m:
        r = g.UInt32.addmany(m, [a, g.UInt32.constant(0x80000001), not_a, g.UInt32.constant(0xFFFFFFFF)])
    assert len(cs.aux_assignment) - before == 34 and r.value == (0xFFFFFFFF + 0x80000001 + 0 + 0xFFFFFFFF) & 0xFFFFFFFF and _satisfied(cs)
    cs = _cs()
    with g.MultiEq(cs) as m:
        r = g.UInt32.addmany(m, [g.UInt32.constant(0xFFFFFFFF), g.UInt32.constant(0x80000001), g.UInt32.constant(7)])
    assert not cs.aux_assignment and not cs.a and r.value == (0xFFFFFFFF + 0x80000001 + 7) & 0xFFFFFFFF and r.is_constant()
    with pytest.raises(AssertionError):
        g.UInt32.addmany(g.MultiEq(_cs()), [g.UInt32.constant(1)])
    with pytest.raises(AssertionError):
        g.UInt32.addmany(g.MultiEq(_cs()), [g.UInt32.constant(1)] * 11)
    cs2 = _cs()   # wrong result bits are caught by the deferred equality
    a2 = g.UInt32.alloc(cs2, 5)
    bad = g.UInt32.from_bits(a2.bits)
    bad.value = 6   # the value the result bits are allocated from
    with g.MultiEq(cs2) as m:
        g.UInt32.addmany(m, [bad, a2])
    assert not _satisfied(cs2)


def test_uint32_rotations_shifts_and_bit_orders():
    cs = _cs()
    v = 0x80000001
    a = g.UInt32.alloc(cs, v)
    for by in (0, 1, 7, 31, 32, 39):
        assert a.rotr(by).value == ((v >> (by % 32)) | (v << (32 - by % 32))) & 0xFFFFFFFF
        assert [b.get_value() for b in a.rotr(by).bits] == [bool((a.rotr(by).value >> i) & 1) for i in range(32)]
        assert a.shr(by).value == v >> (by % 32)
        assert [b.get_value() for b in a.shr(by).bits] == [bool((a.shr(by).value >> i) & 1) for i in range(32)]
    assert g.UInt32.from_bits_be(a.into_bits_be()).value == v and g.UInt32.from_bits(a.into_bits()).value == v
    assert g.UInt32.constant(v).value == v and a.xor(cs, g.UInt32.constant(0xFFFFFFFF)).value == v ^ 0xFFFFFFFF
    assert g.UInt32.alloc(ShapeAssembly(), None).value is None


# ---- MultiEq ---------------------------------------------------------------------------------------------------------------
def test_multieq_emits_at_capacity_and_at_scope_end():
    from bellman_amd.groth16 import LinearCombination

    assert g.CAPACITY == 254
    z = LinearCombination.zero()
    cs = ShapeAssembly()
    with g.MultiEq(cs) as m:
        for _ in range(7):
            m.enforce_equal(36, z, z)
        assert m.bits_used == 252 and len(cs.rows[0]) == 0
        m.enforce_equal(1, z, z)          # 253 < 254: still pending
        assert m.bits_used == 253 and len(cs.rows[0]) == 0
        m.enforce_equal(1, z, z)          # bits_used + n reaches 254: the pending constraint goes out first
        assert len(cs.rows[0]) == 1 and m.bits_used == 1 and m.ops == 1
    assert len(cs.rows[0]) == 2           # ... and the rest at the end of the scope
    cs = ShapeAssembly()
    with g.MultiEq(cs) as m:
        m.enforce_equal(127, z, z)
        m.enforce_equal(127, z, z)        # 127 + 127 = 254
        assert len(cs.rows[0]) == 1
    assert len(cs.rows[0]) == 2
    cs = ShapeAssembly()
    with g.MultiEq(cs):
        pass
    assert len(cs.rows[0]) == 0           # nothing pending, nothing emitted
    with pytest.raises(AssertionError):
        g.MultiEq(ShapeAssembly()).enforce_equal(254, z, z)
    # the scaled sides: the second equality sits 36 bits up
    cs = _cs()
    x = cs.alloc(lambda: 5)
    y = cs.alloc(lambda: 9)
    with g.MultiEq(cs) as m:
        m.enforce_equal(36, z + x, z + x)
        m.enforce_equal(36, z + y, z + y)
    assert cs.a == [5 + (9 << 36)] and cs.c == cs.a and cs.b == [1]


def test_multipacking_helpers():
    assert g.bytes_to_bits(b"\x80\x01") == [True] + [False] * 14 + [True]
    assert g.bytes_to_bits_le(b"\x80\x01") == [False] * 7 + [True, True] + [False] * 7
    bits = [True] * 256
    assert g.compute_multipacking(bits) == [(1 << 254) - 1, 3]
    cs = _cs()
    g.pack_into_inputs(cs, [g.Boolean.Is(g.AllocatedBit.alloc(cs, True)) for _ in range(255)] + [g.Boolean.constant(True)])
    assert cs.input_assignment[1:] == [(1 << 254) - 1, 3] and _satisfied(cs)
