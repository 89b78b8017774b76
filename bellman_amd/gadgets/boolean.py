"""`gadgets::boolean` (reference: src/gadgets/boolean.rs): bits in the circuit and boolean logic, case for case.

Values are None (shape capture) or concrete.  Every operation that may allocate takes `tag`, the record (word, bit, neg) of its
LOGICAL result in the recorded word program (recorder.py): the variable it allocates - whichever folding path gets there - is
bit `bit` of trace word `word`, xor `neg`.  Without a tag (or without a recorder on the constraint system) nothing is recorded."""

from ..groth16 import ConstraintSystem, LinearCombination
from .recorder import flip, recorder_of

CONSTANT, IS, NOT = 0, 1, 2


def _scalar(value):
    """the value closure of a bit: AssignmentMissing (here AssertionError) when the value is called for but unknown"""
    def f():
        assert value is not None, "AssignmentMissing"
        return 1 if value else 0
    return f


def _opt(f, *vals):
    return None if any(v is None for v in vals) else f(*vals)


class AllocatedBit:
    """boolean.rs:11-267: a variable that is guaranteed to be 0 or 1.  `rec`: the variable's record, or None."""

    __slots__ = ("variable", "value", "rec")

    def __init__(self, variable, value, rec=None):
        self.variable, self.value, self.rec = variable, value, rec

    @staticmethod
    def _new(cs, value, tag):
        var = cs.alloc(_scalar(value))
        r = recorder_of(cs)
        if r is not None and tag is not None:
            r.bit_variable(var, tag)
        else:
            tag = None
        return var, AllocatedBit(var, value, tag)

    @staticmethod
    def alloc(cs, value, tag=None):
        """boolean.rs:70-99"""
        var, bit = AllocatedBit._new(cs, value, tag)
        one = ConstraintSystem.one()
        cs.enforce(lambda lc: lc + one - var, lambda lc: lc + var, lambda lc: lc)   # (1 - a) * a = 0
        return bit

    @staticmethod
    def xor(cs, a, b, tag=None):
        """boolean.rs:103-151"""
        var, bit = AllocatedBit._new(cs, _opt(lambda x, y: x ^ y, a.value, b.value), tag)
        cs.enforce(lambda lc: lc + a.variable + a.variable, lambda lc: lc + b.variable,
                   lambda lc: lc + a.variable + b.variable - var)                    # (a + a) * b = a + b - c
        return bit

    @staticmethod
    def and_(cs, a, b, tag=None):
        """boolean.rs:155-190"""
        var, bit = AllocatedBit._new(cs, _opt(lambda x, y: x & y, a.value, b.value), tag)
        cs.enforce(lambda lc: lc + a.variable, lambda lc: lc + b.variable, lambda lc: lc + var)
        return bit

    @staticmethod
    def and_not(cs, a, b, tag=None):
        """boolean.rs:193-228: a AND (NOT b)"""
        var, bit = AllocatedBit._new(cs, _opt(lambda x, y: x & (not y), a.value, b.value), tag)
        one = ConstraintSystem.one()
        cs.enforce(lambda lc: lc + a.variable, lambda lc: lc + one - b.variable, lambda lc: lc + var)
        return bit

    @staticmethod
    def nor(cs, a, b, tag=None):
        """boolean.rs:231-266: (NOT a) AND (NOT b)"""
        var, bit = AllocatedBit._new(cs, _opt(lambda x, y: (not x) & (not y), a.value, b.value), tag)
        one = ConstraintSystem.one()
        cs.enforce(lambda lc: lc + one - a.variable, lambda lc: lc + one - b.variable, lambda lc: lc + var)
        return bit


class Boolean:
    """boolean.rs:360-368: Is(AllocatedBit) / Not(AllocatedBit) / Constant(bool)"""

    __slots__ = ("kind", "bit", "const")

    def __init__(self, kind, bit=None, const=None):
        self.kind, self.bit, self.const = kind, bit, const

    @staticmethod
    def Is(bit):
        return Boolean(IS, bit)

    @staticmethod
    def Not(bit):
        return Boolean(NOT, bit)

    @staticmethod
    def Constant(b):
        return Boolean(CONSTANT, None, bool(b))

    constant = Constant   # boolean.rs:450-452

    def is_constant(self):
        return self.kind == CONSTANT

    def get_value(self):
        """boolean.rs:421-427"""
        if self.kind == CONSTANT:
            return self.const
        v = self.bit.value
        return None if v is None else bool(v) if self.kind == IS else not v

    def tag(self):
        """the record of this Boolean's logical value, or None (a constant, an untagged variable)"""
        if self.kind == CONSTANT or self.bit.rec is None:
            return None
        return self.bit.rec if self.kind == IS else flip(self.bit.rec)

    def lc(self, one, coeff):
        """boolean.rs:429-447"""
        z = LinearCombination.zero()
        if self.kind == CONSTANT:
            return z + (coeff, one) if self.const else z
        if self.kind == IS:
            return z + (coeff, self.bit.variable)
        return z + (coeff, one) - (coeff, self.bit.variable)

    def not_(self):
        """boolean.rs:455-461"""
        if self.kind == CONSTANT:
            return Boolean.Constant(not self.const)
        return Boolean(NOT if self.kind == IS else IS, self.bit)

    @staticmethod
    def xor(cs, a, b, tag=None):
        """boolean.rs:464-483"""
        for x, y in ((a, b), (b, a)):
            if x.kind == CONSTANT and not x.const:
                return y
        for x, y in ((a, b), (b, a)):
            if x.kind == CONSTANT and x.const:
                return y.not_()
        if a.kind != b.kind:   # a XOR (NOT b) = NOT(a XOR b)
            is_, not__ = (a, b) if a.kind == IS else (b, a)
            return Boolean.xor(cs, is_, not__.not_(), flip(tag)).not_()
        return Boolean.Is(AllocatedBit.xor(cs, a.bit, b.bit, tag))   # a XOR b = (NOT a) XOR (NOT b)

    @staticmethod
    def and_(cs, a, b, tag=None):
        """boolean.rs:486-512"""
        if (a.kind == CONSTANT and not a.const) or (b.kind == CONSTANT and not b.const):
            return Boolean.Constant(False)
        for x, y in ((a, b), (b, a)):
            if x.kind == CONSTANT and x.const:
                return y
        if a.kind != b.kind:
            is_, not__ = (a, b) if a.kind == IS else (b, a)
            return Boolean.Is(AllocatedBit.and_not(cs, is_.bit, not__.bit, tag))
        if a.kind == NOT:
            return Boolean.Is(AllocatedBit.nor(cs, a.bit, b.bit, tag))
        return Boolean.Is(AllocatedBit.and_(cs, a.bit, b.bit, tag))

    @staticmethod
    def sha256_ch(cs, a, b, c, tag=None):
        """boolean.rs:515-619: (a and b) xor ((not a) and c)"""
        ch_value = _opt(lambda x, y, z: (x & y) ^ ((not x) & z), a.get_value(), b.get_value(), c.get_value())
        ka, kb, kc = a.kind == CONSTANT, b.kind == CONSTANT, c.kind == CONSTANT
        if ka and kb and kc:
            return Boolean.Constant(ch_value)
        if ka and not a.const:
            return c
        if kb and not b.const:
            return Boolean.and_(cs, a.not_(), c, tag)
        if kc and not c.const:
            return Boolean.and_(cs, a, b, tag)
        if kc and c.const:
            return Boolean.and_(cs, a, b.not_(), flip(tag)).not_()
        if kb and b.const:
            return Boolean.and_(cs, a.not_(), c.not_(), flip(tag)).not_()
        # (a constant true falls through, boolean.rs:580-586)
        var, bit = AllocatedBit._new(cs, ch_value, tag)
        one = ConstraintSystem.one()
        cs.enforce(lambda _: b.lc(one, 1).sub_scaled(1, c.lc(one, 1)), lambda _: a.lc(one, 1),
                   lambda lc: (lc + var).sub_scaled(1, c.lc(one, 1)))                # a(b - c) = ch - c
        return Boolean.Is(bit)

    @staticmethod
    def sha256_maj(cs, a, b, c, tag=None, bc_tag=None):
        """boolean.rs:622-736: (a and b) xor (a and c) xor (b and c).  bc_tag: the record of the intermediate b AND c."""
        maj_value = _opt(lambda x, y, z: (x & y) ^ (x & z) ^ (y & z), a.get_value(), b.get_value(), c.get_value())
        ka, kb, kc = a.kind == CONSTANT, b.kind == CONSTANT, c.kind == CONSTANT
        if ka and kb and kc:
            return Boolean.Constant(maj_value)
        if ka and not a.const:
            return Boolean.and_(cs, b, c, tag)
        if kb and not b.const:
            return Boolean.and_(cs, a, c, tag)
        if kc and not c.const:
            return Boolean.and_(cs, a, b, tag)
        if kc and c.const:
            return Boolean.and_(cs, a.not_(), b.not_(), flip(tag)).not_()
        if kb and b.const:
            return Boolean.and_(cs, a.not_(), c.not_(), flip(tag)).not_()
        if ka and a.const:
            return Boolean.and_(cs, b.not_(), c.not_(), flip(tag)).not_()
        var, bit = AllocatedBit._new(cs, maj_value, tag)
        bc = Boolean.and_(cs, b, c, bc_tag)
        one = ConstraintSystem.one()
        cs.enforce(lambda _: bc.lc(one, 1).add_scaled(1, bc.lc(one, 1)).sub_scaled(1, b.lc(one, 1)).sub_scaled(1, c.lc(one, 1)),
                   lambda _: a.lc(one, 1),
                   lambda _: bc.lc(one, 1) - var)                                    # (2bc - b - c) * a = bc - maj
        return Boolean.Is(bit)
