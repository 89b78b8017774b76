"""`gadgets::multipack` (reference: src/gadgets/multipack.rs:11-72): bits packed into scalar field elements."""

from ..groth16 import ConstraintSystem, LinearCombination, Q
from .multieq import CAPACITY
from .recorder import recorder_of


def pack_into_inputs(cs, bits):
    """multipack.rs:11-37: exposes `bits` as compact public inputs, CAPACITY bits per input.  With a recorder every input is
    recorded as a packed variable: the sum of bit_i * 2^i over the records of its bits."""
    one = ConstraintSystem.one()
    r = recorder_of(cs)
    for lo in range(0, len(bits), CAPACITY):
        chunk = bits[lo:lo + CAPACITY]
        num_lc, num_value = LinearCombination.zero(), 0   # Num::zero, add_bool_with_coeff (num.rs:383-414)
        coeff = 1
        for bit in chunk:
            v = bit.get_value()
            num_value = None if num_value is None or v is None else (num_value + coeff if v else num_value)
            num_lc = num_lc.add_scaled(1, bit.lc(one, coeff))
            coeff = coeff * 2 % Q

        def value(num_value=num_value):
            assert num_value is not None, "AssignmentMissing"
            return num_value

        inp = cs.alloc_input(value)
        if r is not None:
            r.packed_variable(inp, [r.bit_source(b) for b in chunk])
        cs.enforce(lambda _: LinearCombination.zero().add_scaled(1, num_lc), lambda lc: lc + one, lambda lc: lc + inp)   # num * 1 = input


def bytes_to_bits(data):
    """multipack.rs:39-44: most significant bit of every byte first"""
    return [bool((v >> i) & 1) for v in bytes(data) for i in range(7, -1, -1)]


def bytes_to_bits_le(data):
    """multipack.rs:46-51"""
    return [bool((v >> i) & 1) for v in bytes(data) for i in range(8)]


def compute_multipacking(bits):
    """multipack.rs:53-72 -> ints in [0, q)"""
    out = []
    for lo in range(0, len(bits), CAPACITY):
        out.append(sum(1 << i for i, b in enumerate(bits[lo:lo + CAPACITY]) if b) % Q)
    return out
