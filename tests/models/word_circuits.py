"""One-op circuits for the word-program tests: one circuit per instruction kind of the recorded program (bellman_amd/gadgets),
a few hundred variables each.  Every circuit allocates its external words first (UInt32.alloc: 32 aux bits per word) and builds
its operands from them with Is, Not and constant bits mixed, so that every folding path of the Boolean gadgets is taken and the
operand words reach the program through PACK.  A circuit is a callable; `with_ext(row)` gives the copy that carries values."""

import random

import numpy as np

from bellman_amd import gadgets as g

SPECIAL = (0, 0xFFFFFFFF, 0x80000001)


def mixed(u, pattern):
    """a UInt32 over u's variables with Is, Not and constant bits mixed (deterministic in `pattern`)"""
    bits = []
    for i, b in enumerate(u.bits):
        sel = (i * 7 + pattern * 3 + (i >> 3)) % 5
        bits.append(b if sel in (0, 3) else b.not_() if sel in (1, 4) else g.Boolean.constant((i + pattern) & 1))
    return g.UInt32.from_bits(bits)


class OneOp:
    N_EXT = {"xor": 2, "rotr_xor": 2, "shr_xor": 2, "ch": 3, "maj": 3, "add2": 2, "add5": 4, "add10": 10, "pack": 2, "packed_input": 8}

    def __init__(self, kind, ext=None):
        self.kind, self.n_ext, self.ext = kind, self.N_EXT[kind], ext

    def with_ext(self, row):
        assert len(row) == self.n_ext
        return OneOp(self.kind, [int(x) for x in row])

    def __call__(self, cs):
        w = [g.UInt32.alloc(cs, v) for v in (self.ext or [None] * self.n_ext)]
        kind = self.kind
        if kind == "xor":
            w[0].xor(cs, w[1])
            mixed(w[0], 1).xor(cs, mixed(w[1], 2))
        elif kind == "rotr_xor":
            w[0].rotr(7).xor(cs, w[1].rotr(18))
            mixed(w[0], 3).rotr(13).xor(cs, mixed(w[1], 4).rotr(31))
        elif kind == "shr_xor":
            w[0].shr(3).xor(cs, w[1])
            mixed(w[0], 5).shr(10).xor(cs, mixed(w[1], 6).shr(1))
        elif kind == "ch":
            g.UInt32.sha256_ch(cs, w[0], w[1], w[2])
            g.UInt32.sha256_ch(cs, mixed(w[0], 1), mixed(w[1], 2), mixed(w[2], 4))
        elif kind == "maj":
            g.UInt32.sha256_maj(cs, w[0], w[1], w[2])
            g.UInt32.sha256_maj(cs, mixed(w[0], 2), mixed(w[1], 3), mixed(w[2], 0))
        elif kind in ("add2", "add5", "add10"):
            with g.MultiEq(cs) as m:
                if kind == "add2":
                    g.UInt32.addmany(m, [w[0], w[1]])
                    g.UInt32.addmany(m, [mixed(w[0], 1), g.UInt32.constant(0xFFFFFFFF)])
                elif kind == "add5":
                    g.UInt32.addmany(m, [w[0], mixed(w[1], 2), g.UInt32.constant(0x80000001), w[2].rotr(5), w[3]])
                else:
                    g.UInt32.addmany(m, w)
                    g.UInt32.addmany(m, [mixed(x, i) for i, x in enumerate(w)])
        elif kind == "pack":
            # halves of two words, a negated nibble and two constants: no aligned image of one word
            bits = w[0].bits[:16] + [b.not_() for b in w[1].bits[16:20]] + w[1].bits[20:30] + [g.Boolean.constant(True), g.Boolean.constant(False)]
            g.UInt32.from_bits(bits).xor(cs, w[1])
            g.UInt32.from_bits_be(bits).rotr(9).xor(cs, w[0])
        else:   # packed_input: 256 bits -> one input of 254 bits and one of 2
            g.pack_into_inputs(cs, [b for x in w for b in x.bits])


KINDS = tuple(OneOp.N_EXT)


def ext_rows(kind, k, seed=7):
    """[k, n_ext] uint32: all-zero, all-ones (for packed_input the all-ones 254-bit pack, 2^254 - 1 < q), 0x80000001
    throughout, the three rotated through the words, then random words"""
    n = OneOp.N_EXT[kind]
    rnd = random.Random(seed * 1000 + n)
    rows = [[s] * n for s in SPECIAL] + [[SPECIAL[(e + r) % 3] for e in range(n)] for r in range(3)]
    while len(rows) < k:
        rows.append([rnd.getrandbits(32) for _ in range(n)])
    return np.array(rows[:k], dtype=np.uint32)


def host_witnesses(circuit_with, rows):
    """host synthesis per row -> ([k, n_inputs, 4], [k, n_aux, 4]) uint64 Montgomery"""
    from bellman_amd.groth16 import fr_to_mont_array

    ins, auxs = [], []
    for row in rows:
        i, a = g.synthesize(circuit_with(row))
        ins.append(fr_to_mont_array(i))
        auxs.append(fr_to_mont_array(a))
    return np.stack(ins), np.stack(auxs)
