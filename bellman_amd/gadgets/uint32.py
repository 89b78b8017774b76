"""`gadgets::uint32` (reference: src/gadgets/uint32.rs): 32 Booleans read as an unsigned integer, least significant first.

With a recorder on the constraint system every operation appends the instruction that computes its result word and tags the
Booleans it makes with (that word, bit, 0).  A UInt32 learns its own trace word lazily (`word`): a constant is a CONST, a
rotation or shift one instruction on its parent's word, 32 bits that are bit i of ONE word at position i are that word, anything
else is a PACK of its 32 bit sources."""

from ..groth16 import ConstraintSystem, LinearCombination
from . import recorder as rc
from .boolean import AllocatedBit, Boolean
from .recorder import recorder_of

_M32 = 0xFFFFFFFF


class UInt32:
    __slots__ = ("bits", "value", "_word", "_lazy")

    def __init__(self, bits, value, word=None, lazy=None):
        self.bits, self.value, self._word, self._lazy = bits, value, word, lazy

    @staticmethod
    def constant(value):
        """uint32.rs:25-43"""
        return UInt32([Boolean.constant((value >> i) & 1) for i in range(32)], value & _M32)

    @staticmethod
    def alloc(cs, value):
        """uint32.rs:46-77; with a recorder the 32 bits are a new external word"""
        r = recorder_of(cs)
        w = r.external() if r is not None else None
        bits = [Boolean.Is(AllocatedBit.alloc(cs, None if value is None else (value >> i) & 1, (w, i, 0) if r is not None else None))
                for i in range(32)]
        return UInt32(bits, value, word=w)

    def into_bits_be(self):
        """uint32.rs:79-83"""
        return self.bits[::-1]

    @staticmethod
    def from_bits_be(bits):
        """uint32.rs:85-111"""
        return UInt32.from_bits(list(bits)[::-1])

    def into_bits(self):
        """uint32.rs:114-116"""
        return list(self.bits)

    @staticmethod
    def from_bits(bits):
        """uint32.rs:120-164"""
        bits = list(bits)
        assert len(bits) == 32
        value = 0
        for i, b in enumerate(bits):
            v = b.get_value()
            if v is None:
                value = None
                break
            value |= int(v) << i
        return UInt32(bits, value)

    def rotr(self, by):
        """uint32.rs:166-182"""
        by %= 32
        v = None if self.value is None else ((self.value >> by) | (self.value << (32 - by))) & _M32
        return UInt32((self.bits[by:] + self.bits)[:32], v, lazy=(rc.ROTR, self, by) if by else (None, self, 0))

    def shr(self, by):
        """uint32.rs:184-202"""
        by %= 32
        fill = Boolean.constant(False)
        return UInt32((self.bits[by:] + [fill] * 32)[:32], None if self.value is None else self.value >> by,
                      lazy=(rc.SHR, self, by) if by else (None, self, 0))

    def is_constant(self):
        return all(b.is_constant() for b in self.bits)

    def word(self, r):
        """this value's trace word id in recorder r (instructions are appended as needed), or None when a bit has no record"""
        if self._word is None:
            if self.is_constant():
                self._word = r.const(self.value)
            elif self._lazy is not None:
                op, parent, by = self._lazy
                self._word = parent.word(r) if op is None else r.emit(op, parent.word(r), by)
            else:
                tags = [b.tag() for b in self.bits]
                if all(t is not None and t[0] == tags[0][0] and t[1] == i and t[2] == 0 for i, t in enumerate(tags)):
                    self._word = tags[0][0]   # an aligned image of one word
                else:
                    self._word = r.emit(rc.PACK, [r.bit_source(b) for b in self.bits])
        return self._word

    @staticmethod
    def _op_word(cs, op, operands):
        """the word of `op` over `operands`, or None: no recorder, or every operand constant (so is the result)"""
        r = recorder_of(cs)
        if r is None or all(o.is_constant() for o in operands):
            return None
        return r.emit(op, *[o.word(r) for o in operands])

    @staticmethod
    def _triop(cs, a, b, c, value_fn, circuit_fn, op):
        """uint32.rs:204-236"""
        value = None if None in (a.value, b.value, c.value) else value_fn(a.value, b.value, c.value) & _M32
        w = UInt32._op_word(cs, op, (a, b, c))
        bits = [circuit_fn(cs, i, x, y, z, None if w is None else (w, i, 0)) for i, (x, y, z) in enumerate(zip(a.bits, b.bits, c.bits))]
        return UInt32(bits, value, word=w)

    @staticmethod
    def sha256_maj(cs, a, b, c):
        """uint32.rs:240-258; the intermediate b AND c of the general case is a word of its own"""
        bc = UInt32._op_word(cs, rc.AND, (b, c))
        return UInt32._triop(cs, a, b, c, lambda x, y, z: (x & y) ^ (x & z) ^ (y & z),
                             lambda cs, i, x, y, z, t: Boolean.sha256_maj(cs, x, y, z, t, None if bc is None or t is None else (bc, i, 0)),
                             rc.MAJ)

    @staticmethod
    def sha256_ch(cs, a, b, c):
        """uint32.rs:262-280"""
        return UInt32._triop(cs, a, b, c, lambda x, y, z: (x & y) ^ (~x & z),
                             lambda cs, i, x, y, z, t: Boolean.sha256_ch(cs, x, y, z, t), rc.CH)

    def xor(self, cs, other):
        """uint32.rs:283-305"""
        value = None if None in (self.value, other.value) else self.value ^ other.value
        w = UInt32._op_word(cs, rc.XOR, (self, other))
        bits = [Boolean.xor(cs, x, y, None if w is None else (w, i, 0)) for i, (x, y) in enumerate(zip(self.bits, other.bits))]
        return UInt32(bits, value, word=w)

    @staticmethod
    def addmany(cs, operands):
        """uint32.rs:308-408; `cs` is a MultiEq (multieq.py), which takes the equality"""
        assert 2 <= len(operands) <= 10
        max_value = len(operands) * _M32
        result_value = 0
        one = ConstraintSystem.one()
        lc = LinearCombination.zero()
        all_constants = True
        for op in operands:
            result_value = None if result_value is None or op.value is None else result_value + op.value
            coeff = 1
            for bit in op.bits:
                lc = lc.add_scaled(1, bit.lc(one, coeff))
                all_constants &= bit.is_constant()
                coeff *= 2
        if all_constants and result_value is not None:
            return UInt32.constant(result_value & _M32)
        r = recorder_of(cs)
        words = [op.word(r) for op in operands] if r is not None else None
        s = r.emit(rc.ADD, words) if r is not None else None   # the full sum, up to 36 bits
        result_bits = []
        result_lc = LinearCombination.zero()
        coeff, i = 1, 0
        while max_value != 0:
            b = AllocatedBit.alloc(cs, None if result_value is None else (result_value >> i) & 1, None if s is None else (s, i, 0))
            result_lc = result_lc + (coeff, b.variable)
            result_bits.append(Boolean.Is(b))
            max_value >>= 1
            i += 1
            coeff *= 2
        if r is not None:
            r.hints.append((lc, [b.bit.variable for b in result_bits]))
        cs.enforce_equal(i, lc, result_lc)
        return UInt32(result_bits[:32], None if result_value is None else result_value & _M32, word=s)
