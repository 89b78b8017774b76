"""`gadgets::multieq` (reference: src/gadgets/multieq.rs): several equalities of small bit width folded into one constraint.

The reference emits the pending constraint when the MultiEq is dropped; here the scope is a `with` block (or `close()`)."""

from ..groth16 import ConstraintSystem, LinearCombination

CAPACITY = 254   # Scalar::CAPACITY of bls12_381::Scalar


class MultiEq(ConstraintSystem):
    def __init__(self, cs):
        """multieq.rs:14-22"""
        self.cs = cs
        self.ops = 0
        self.bits_used = 0
        self.lhs, self.rhs = LinearCombination.zero(), LinearCombination.zero()

    @property
    def recorder(self):
        return getattr(self.cs, "recorder", None)

    def accumulate(self):
        """multieq.rs:24-38"""
        lhs, rhs = self.lhs, self.rhs
        one = ConstraintSystem.one()
        self.cs.enforce(lambda _: lhs, lambda lc: lc + one, lambda _: rhs)
        self.lhs, self.rhs = LinearCombination.zero(), LinearCombination.zero()
        self.bits_used = 0
        self.ops += 1

    def enforce_equal(self, num_bits, lhs, rhs):
        """multieq.rs:40-57"""
        if CAPACITY <= self.bits_used + num_bits:
            self.accumulate()
        assert CAPACITY > self.bits_used + num_bits
        coeff = 1 << self.bits_used
        self.lhs = self.lhs.add_scaled(coeff, lhs)
        self.rhs = self.rhs.add_scaled(coeff, rhs)
        self.bits_used += num_bits

    def close(self):
        """multieq.rs:60-66 (Drop)"""
        if self.bits_used > 0:
            self.accumulate()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False

    # multieq.rs:68-121: everything else goes to the wrapped constraint system
    def alloc(self, f):
        return self.cs.alloc(f)

    def alloc_input(self, f):
        return self.cs.alloc_input(f)

    def enforce(self, a, b, c):
        return self.cs.enforce(a, b, c)
