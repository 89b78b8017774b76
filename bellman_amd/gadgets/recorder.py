"""The word program the gadgets imply: a straight-line program over TRACE WORDS (u64; the 32-bit operations read the low 32
bits of their sources) that computes, for one witness, every word whose bits the circuit's variables are.

While a circuit is synthesised the recorder names words by ids: external word e (preloaded per witness) is -(e + 1), the result
of instruction j is j.  `finish` turns them into indices - externals first, then one word per instruction - and the records into
the arrays of bh_word_witness_desc (include/bellman_hip.h)."""

import numpy as np

from .._abi import C
from ..groth16 import INPUT

CONST, ROTR, SHR, XOR, AND, CH, MAJ, ADD, PACK = (getattr(C, "BH_WORD_" + x) for x in (
    "CONST", "ROTR", "SHR", "XOR", "AND", "CH", "MAJ", "ADD", "PACK"))
MAX_PACKED_BITS = 254                                            # Scalar::CAPACITY


def recorder_of(cs):
    return getattr(cs, "recorder", None)


def flip(tag):
    return None if tag is None else (tag[0], tag[1], tag[2] ^ 1)


class Recorder:
    def __init__(self):
        self.n_ext = 0
        self.instrs = []       # (op, payload)
        self.bit_vars = {}     # (kind, idx) -> (word id, bit, neg)
        self.packed = []       # ((kind, idx), [(word id, bit, neg)])
        self.hints = []        # (LinearCombination, [Variable]): the result bits of one addmany
        self._consts = {}

    def external(self):
        """a new external word: its 32 bits are the caller's, one uint32 per witness"""
        self.n_ext += 1
        return -self.n_ext

    def emit(self, op, *payload):
        """the id of the new word, or None when a source is unknown (an operand built from untagged variables)"""
        if any(p is None for p in payload) or any(p is None for p in (payload[0] if op in (ADD, PACK) else ())):
            return None
        self.instrs.append((op, payload))
        return len(self.instrs) - 1

    def const(self, value):
        if value not in self._consts:
            self._consts[value] = self.emit(CONST, value)
        return self._consts[value]

    def bit_source(self, boolean):
        """(word id, bit, neg) whose value is `boolean`'s; a constant is bit 0 of the zero word, negated for true"""
        if boolean.is_constant():
            return (self.const(0), 0, 1 if boolean.const else 0)
        return boolean.tag()

    def bit_variable(self, var, tag):
        self.bit_vars[(var.kind, var.idx)] = tag

    def packed_variable(self, var, sources):
        if all(s is not None for s in sources):
            self.packed.append(((var.kind, var.idx), list(sources)))

    def finish(self, num_inputs, num_aux):
        """-> dict of numpy arrays in the layout of bh_word_witness_desc, plus `untagged`: the variables (bh_csr.var numbering)
        no record covers"""
        n_ext = self.n_ext
        word = lambda w: -w - 1 if w < 0 else n_ext + w                 # noqa: E731
        vidx = lambda kv: kv[1] if kv[0] == INPUT else num_inputs + kv[1]   # noqa: E731
        instrs = np.zeros((len(self.instrs), 4), dtype=np.uint32)
        pool, bits = [], []

        def push_bits(sources):
            begin = len(bits)
            bits.extend((word(w), b | (n << 8)) for w, b, n in sources)
            return begin

        for j, (op, p) in enumerate(self.instrs):
            if op == CONST:
                instrs[j] = (op, p[0], 0, 0)
            elif op in (ROTR, SHR):
                instrs[j] = (op, word(p[0]), p[1], 0)
            elif op in (XOR, AND):
                instrs[j] = (op, word(p[0]), word(p[1]), 0)
            elif op in (CH, MAJ):
                instrs[j] = (op, word(p[0]), word(p[1]), word(p[2]))
            elif op == ADD:
                instrs[j] = (op, len(pool), len(p[0]), 0)
                pool.extend(word(w) for w in p[0])
            else:
                instrs[j] = (op, push_bits(p[0]), 0, 0)
        bit_vars = np.array([(vidx(kv), word(w), b | (n << 8)) for kv, (w, b, n) in self.bit_vars.items()],
                            dtype=np.uint32).reshape(-1, 3)
        packed = np.array([(vidx(kv), push_bits(src), len(src)) for kv, src in self.packed], dtype=np.uint32).reshape(-1, 3)
        covered = np.zeros(num_inputs + num_aux, dtype=bool)
        covered[0] = True
        covered[bit_vars[:, 0]] = True
        covered[packed[:, 0]] = True
        return dict(n_ext=n_ext, instrs=instrs, pool=np.array(pool, dtype=np.uint32), bits=np.array(bits, dtype=np.uint32).reshape(-1, 2),
                    bit_vars=bit_vars, packed=packed, untagged=[int(v) for v in np.nonzero(~covered)[0]])
