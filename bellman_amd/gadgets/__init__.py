"""bellman's gadget layer (reference: src/gadgets/) for the SHA-256 family, over the Python ConstraintSystem classes of
bellman_amd.groth16 - and the word program the gadgets record, which the device runs for k witnesses at once
(bh_word_witness_generate_dev; csrc/word_witness.hip) in place of the value closures of prover.rs:206.

    shape = gadgets.capture(Sha256Preimage(55))          # one synthesis: matrices, program, variable records
    r1cs = shape.r1cs(worker)
    gen = shape.witness_generator(worker)
    wit = gen.generate_dev(circuit.ext_from_messages(msgs))   # DeviceWitnesses, as prove_witness_batch_dev reads them
"""

import ctypes

import numpy as np

from .. import _abi, _lib
from .._abi import C
from ..errors import check
from ..groth16 import INPUT, BitsHint, DeviceWitnesses, R1CS, ShapeAssembly, Variable, WitnessAssignment
from .boolean import AllocatedBit, Boolean
from .multieq import CAPACITY, MultiEq
from .multipack import bytes_to_bits, bytes_to_bits_le, compute_multipacking, pack_into_inputs
from .recorder import Recorder
from .sha256 import Sha256Preimage, sha256, sha256_block_no_padding, sha256_compression_function
from .uint32 import UInt32

__all__ = ["AllocatedBit", "Boolean", "UInt32", "MultiEq", "CAPACITY", "pack_into_inputs", "bytes_to_bits", "bytes_to_bits_le",
           "compute_multipacking", "sha256", "sha256_block_no_padding", "sha256_compression_function", "Sha256Preimage",
           "Recorder", "RecordingShape", "Shape", "WordWitness", "WordProgramError", "capture", "synthesize"]

# BH_WORD_BAD_*: why bh_word_witness_create refused a program, and what the index it reports counts
BAD_SOURCE, BAD_BIT, BAD_ADD_ARITY, BAD_OP, BAD_VAR_SOURCE, BAD_PACKED_BITS, BAD_VAR_RANGE, BAD_UNCOVERED, BAD_COVERED_TWICE = (
    getattr(C, "BH_WORD_BAD_" + x) for x in ("SOURCE", "BIT", "ADD_ARITY", "OP", "VAR_SOURCE", "PACKED_BITS", "VAR_RANGE", "UNCOVERED",
                                             "COVERED_TWICE"))
_BAD_TEXT = {
    BAD_SOURCE: "instruction %d reads a word that is not strictly earlier than its own",
    BAD_BIT: "instruction %d (a PACK) reads a bit index of 64 or more",
    BAD_ADD_ARITY: "instruction %d (an ADD) has fewer than 2 or more than 10 sources",
    BAD_OP: "instruction %d is malformed (unknown operation, shift amount or a range outside its pool)",
    BAD_VAR_SOURCE: "the record of variable %d names a word or a bit that does not exist",
    BAD_PACKED_BITS: "the packed variable %d has more than 254 bits",
    BAD_VAR_RANGE: "record %d (bit records first, packed records behind them) names a variable out of range",
    BAD_UNCOVERED: "variable %d has no record",
    BAD_COVERED_TWICE: "variable %d has two records (ONE is written by the generator itself)",
}


class WordProgramError(ValueError):
    """a word program the validator (csrc/word_program.hpp) refused: `.code` = BAD_*, `.index` = what that code counts"""

    def __init__(self, code, index):
        ValueError.__init__(self, "word program refused: " + (_BAD_TEXT.get(code, "code %d, index %%d" % code) % index))
        self.code, self.index = code, index


_Desc = _abi.STRUCTS["bh_word_witness_desc"]


def make_desc(num_inputs, num_aux, program):
    """bh_word_witness_desc over the arrays of `program` (Recorder.finish, or hand-made arrays of the same layout)
    -> (the structure, the arrays it points into: keep them alive)"""
    keep = [np.ascontiguousarray(program[name], dtype=np.uint32).reshape(-1, width)
            for name, width in (("instrs", 4), ("pool", 1), ("bits", 2), ("bit_vars", 3), ("packed", 3))]
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    args = [num_inputs, num_aux, int(program["n_ext"])]
    for a in keep:
        args += [ptr(a), a.shape[0]]
    return _Desc(*args), keep


def _load():
    return _lib.load()


def check_program(num_inputs, num_aux, program):
    """the validator alone, without a context (bh_test_word_program): raises WordProgramError"""
    desc, keep = make_desc(num_inputs, num_aux, program)
    bad = (ctypes.c_uint32 * 2)()
    rc = _load().bh_test_word_program(ctypes.byref(desc), bad, None, None, None, None)
    del keep
    if rc == C.BH_ERR_INVALID_ARG and bad[0]:
        raise WordProgramError(int(bad[0]), int(bad[1]))
    check(rc, "word program")


def interpret(num_inputs, num_aux, program, ext_row):
    """one witness by the HOST interpreter of csrc/word_program.hpp (no GPU): ([num_inputs, 4], [num_aux, 4]) uint64
    Montgomery, and the trace words (uint64)"""
    desc, keep = make_desc(num_inputs, num_aux, program)
    ext = np.ascontiguousarray(ext_row, dtype=np.uint32).reshape(-1)
    assert ext.size == int(program["n_ext"]), "one uint32 per external word"
    ins, aux = np.zeros((num_inputs, 4), dtype=np.uint64), np.zeros((num_aux, 4), dtype=np.uint64)
    words = np.zeros(ext.size + keep[0].shape[0], dtype=np.uint64)
    bad = (ctypes.c_uint32 * 2)()
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    rc = _load().bh_test_word_program(ctypes.byref(desc), bad, p(ext), p(ins), p(aux), p(words))
    del keep
    if rc == C.BH_ERR_INVALID_ARG and bad[0]:
        raise WordProgramError(int(bad[0]), int(bad[1]))
    check(rc, "word program")
    return ins, aux, words


class WordWitness:
    """bh_word_witness: a validated word program on the device.  One handle serves one call at a time (it owns the scratch
    word file the calls reuse)."""

    def __init__(self, worker, num_inputs, num_aux, program):
        lib = _load()
        self.worker, self.num_inputs, self.num_aux, self.n_ext = worker, num_inputs, num_aux, int(program["n_ext"])
        desc, keep = make_desc(num_inputs, num_aux, program)
        bad, h = (ctypes.c_uint32 * 2)(), ctypes.c_void_p()
        rc = lib.bh_word_witness_create(worker.ctx, ctypes.byref(desc), ctypes.byref(h), bad)
        del keep
        self._h = None
        if rc == C.BH_ERR_INVALID_ARG and bad[0]:
            raise WordProgramError(int(bad[0]), int(bad[1]))
        check(rc, "WordWitness")
        self._h = h

    def _ext(self, ext):
        ext = np.ascontiguousarray(ext, dtype=np.uint32)
        if ext.ndim != 2 or ext.shape[1] != self.n_ext:
            raise ValueError("ext: a [k, %d] uint32 array, one row of external words per witness" % self.n_ext)
        return ext

    def generate_dev(self, ext, stride_extra=0, stream=None, _chunk=None):
        """k witnesses from their external words, on the device: -> DeviceWitnesses (owned by the caller) that
        R1CS.which_is_unsatisfied-style checks, Solver.solve_many_dev and prove_witness_batch_dev read in place.
        stride_extra: bytes of padding behind every vector (a multiple of 32; filled with DeviceWitnesses.from_host's pattern
        and never written).  _chunk: witnesses per scratch chunk for this handle from now on (bh_test_word_witness_chunk)."""
        lib = _load()
        ext = self._ext(ext)
        k = ext.shape[0]
        if stride_extra or k == 0:
            w = DeviceWitnesses.from_host(self.worker, np.zeros((k, self.num_inputs, 4), dtype=np.uint64),
                                          np.zeros((k, self.num_aux, 4), dtype=np.uint64), stride_extra)
        else:   # every variable is written: nothing to upload
            bufs = []
            for n in (self.num_inputs, self.num_aux):
                b = ctypes.c_void_p()
                check(lib.bh_dev_alloc(self.worker.ctx, max(k * n * 32, 32), ctypes.byref(b)), "WordWitness.generate_dev")
                bufs.append(b)
            w = DeviceWitnesses(self.worker, bufs[0], self.num_inputs * 32, bufs[1], self.num_aux * 32, k, self.num_inputs, self.num_aux)
        if _chunk is not None:
            check(lib.bh_test_word_witness_chunk(self._h, _chunk), "WordWitness")
        if k == 0:
            return w
        d = ctypes.c_void_p()
        check(lib.bh_dev_alloc(self.worker.ctx, max(ext.nbytes, 32), ctypes.byref(d)), "WordWitness.generate_dev")
        try:
            if ext.nbytes:
                check(lib.bh_dev_upload(self.worker.ctx, d, ext.ctypes.data_as(ctypes.c_void_p), ext.nbytes), "WordWitness.generate_dev")
            self.generate_into(d, self.n_ext * 4, w, stream)
            if stream is not None:
                check(lib.bh_stream_synchronize(self.worker.ctx, stream), "WordWitness.generate_dev")
            else:
                check(lib.bh_ctx_synchronize(self.worker.ctx), "WordWitness.generate_dev")   # `d` is freed below
        finally:
            lib.bh_dev_free(self.worker.ctx, d)
        return w

    def generate_into(self, ext_dev, ext_stride, dev_witnesses, stream=None):
        """bh_word_witness_generate_dev as it is: external words already on the device (witness j's at ext_dev + j *
        ext_stride bytes), the witnesses written into existing DeviceWitnesses; asynchronous on `stream`"""
        w = dev_witnesses
        if (w.n_inputs, w.n_aux) != (self.num_inputs, self.num_aux):
            raise ValueError("witness buffers of another circuit")
        check(_load().bh_word_witness_generate_dev(self.worker.ctx, self._h, ext_dev, ext_stride, w.inputs, w.in_stride, w.aux,
                                                   w.aux_stride, w.k, stream), "WordWitness.generate_dev")

    def generate(self, ext):
        """the same from and to host arrays (bh_word_witness_generate): ([k, num_inputs, 4], [k, num_aux, 4]) uint64 Montgomery"""
        ext = self._ext(ext)
        k = ext.shape[0]
        ins, aux = np.zeros((k, self.num_inputs, 4), dtype=np.uint64), np.zeros((k, self.num_aux, 4), dtype=np.uint64)
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        check(_load().bh_word_witness_generate(self.worker.ctx, self._h, p(ext), p(ins), p(aux), k), "WordWitness.generate")
        return ins, aux

    def release(self):
        if self._h:
            if getattr(self.worker, "_ctx", None):   # as R1CS.release: the pool is gone with the Worker
                _load().bh_word_witness_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class RecordingShape(ShapeAssembly):
    """ShapeAssembly that carries a Recorder: the gadgets find it as `cs.recorder`"""

    def __init__(self):
        ShapeAssembly.__init__(self)
        self.recorder = Recorder()


class Shape:
    """What one synthesis of a gadget circuit gives (capture): the matrices (`csr()` for R1CS.from_csr) and counts, the
    word `program` (the arrays of bh_word_witness_desc), `untagged` (variables without a record: the program cannot serve
    such a circuit, the solver can), and for R1CS.solver `supplied` (the bits of the external words) and `hints` (one
    BitsHint per non-constant addmany)."""

    def __init__(self, cs):
        self.cs = cs
        self.num_inputs, self.num_aux, self.num_constraints = cs.num_inputs, cs.num_aux, len(cs.rows[0])
        r = cs.recorder
        self.program = r.finish(cs.num_inputs, cs.num_aux)
        self.n_ext, self.untagged = self.program["n_ext"], self.program["untagged"]
        var = lambda kv: Variable(kv[0], kv[1])  # noqa: E731
        self.supplied = [var(kv) for kv, (w, _, _) in r.bit_vars.items() if w < 0]
        self.hints = [BitsHint(lc, outs) for lc, outs in r.hints]

    def csr(self):
        return self.cs.csr()

    def r1cs(self, worker):
        matrices, table = self.cs.csr()
        return R1CS.from_csr(worker, self.num_inputs, self.num_aux, matrices, table)

    def witness_generator(self, worker):
        if self.untagged:
            raise WordProgramError(BAD_UNCOVERED, self.untagged[0])
        return WordWitness(worker, self.num_inputs, self.num_aux, self.program)

    def solver(self, r1cs):
        return r1cs.solver(self.supplied, self.hints)

    def check_program(self):
        check_program(self.num_inputs, self.num_aux, self.program)

    def interpret(self, ext_row):
        """one witness by the host interpreter: ([num_inputs, 4], [num_aux, 4]) uint64 Montgomery"""
        return interpret(self.num_inputs, self.num_aux, self.program, ext_row)[:2]


def capture(circuit):
    """synthesises `circuit` once, structure only, with a recorder -> Shape"""
    cs = RecordingShape()
    cs.alloc_input(lambda: 1)
    circuit(cs)
    for i in range(cs.num_inputs):   # prover.rs:208-215
        cs.enforce(lambda lc, i=i: lc + Variable(INPUT, i), lambda lc: lc, lambda lc: lc)
    return Shape(cs)


def synthesize(circuit):
    """host synthesis of a circuit that carries values, as create_proof_r1cs does it -> (input_assignment, aux_assignment)
    as lists of ints: what the device witnesses are compared with"""
    w = WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return w.input_assignment, w.aux_assignment
