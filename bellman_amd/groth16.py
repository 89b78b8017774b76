"""`groth16::create_proof` mirror (reference: groth16/src/prover.rs:19-361) for Python callers.

Circuits are written against `ConstraintSystem` exactly like bellman user code; synthesis and
linear-combination evaluation run on the host (as in the reference), everything after
`circuit.synthesize` - the h-polynomial FFT pipeline and the eight multiexps - runs on the GPU
through bh_groth16_prove_assignment.  Field elements are Python ints in [0, q).
"""

import ctypes

import numpy as np

from . import _abi, _lib
from ._abi import C
from .errors import UnexpectedEof, Unsatisfiable, check

_check_rc = check  # prove_witness_batch has a keyword argument named `check`

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
_R = (1 << 256) % Q
_MASK = (1 << 64) - 1
INPUT, AUX = 0, 1
STEP_VALIDATE_POINTS = C.BH_STEP_VALIDATE_POINTS
(STEP_FAILED_SHAPE, STEP_FAILED_HEAD, STEP_FAILED_KEY, STEP_FAILED_A, STEP_FAILED_B_G1, STEP_FAILED_B_G2, STEP_FAILED_DELTA, STEP_FAILED_H,
 STEP_FAILED_L, STEP_FAILED_POINTS) = (getattr(C, "BH_STEP_FAILED_" + x) for x in (
     "SHAPE", "HEAD", "KEY", "A", "B_G1", "B_G2", "DELTA", "H", "L", "POINTS"))
# bh_params_step_report: `failed` = the STEP_FAILED_* bits; `bad_vector` (0 key, 1 a, 2 b_g1, 3 b_g2; with
# STEP_FAILED_POINTS 4 h, 5 l, 6 delta_g1, 7 delta_g2) and `bad_index` name the first finding that has a position
ParamsStepReport = _abi.STRUCTS["bh_params_step_report"]


def fr_to_mont_array(vals):
    """ints in [0,q) -> [n,4] uint64 Montgomery limbs (the bytes of bls12_381::Scalar).  An [n,4] uint64 array is
    taken as already converted (callers that prove many times convert their constants once)."""
    if isinstance(vals, np.ndarray) and vals.dtype == np.uint64 and vals.ndim == 2 and vals.shape[1] == 4:
        return np.ascontiguousarray(vals)
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (v % Q) * _R % Q
        out[i] = [(m >> (64 * k)) & _MASK for k in range(4)]
    return out


class Variable:
    """src/lib.rs:163-185"""

    __slots__ = ("kind", "idx")

    def __init__(self, kind, idx):
        self.kind, self.idx = kind, idx


class LinearCombination:
    """src/lib.rs:190-300: ordered (variable, coeff) terms, duplicates not merged."""

    def __init__(self, terms=None):
        self.terms = list(terms or [])

    @staticmethod
    def zero():
        return LinearCombination()

    def __add__(self, other):
        coeff, var = (1, other) if isinstance(other, Variable) else other
        return LinearCombination(self.terms + [(var, coeff % Q)])

    def __sub__(self, other):
        coeff, var = (1, other) if isinstance(other, Variable) else other
        return LinearCombination(self.terms + [(var, (-coeff) % Q)])

    def add_scaled(self, coeff, other):
        """`self + (coeff, &other)` (src/lib.rs:263-280): every term of `other` times coeff, appended in order"""
        coeff %= Q
        return LinearCombination(self.terms + [(var, k * coeff % Q) for var, k in other.terms])

    def sub_scaled(self, coeff, other):
        """`self - (coeff, &other)` (src/lib.rs:282-299)"""
        return self.add_scaled(-coeff, other)


class ConstraintSystem:
    """src/lib.rs:374-437 (subset used by circuits: one, alloc, alloc_input, enforce)."""

    @staticmethod
    def one():
        return Variable(INPUT, 0)


class _Density:
    """src/multiexp.rs:117-157"""

    def __init__(self):
        self.bv = []

    def add_element(self):
        self.bv.append(False)

    def inc(self, i):
        self.bv[i] = True

    def get_total_density(self):
        return sum(self.bv)

    def words(self):
        n = len(self.bv)
        padded = np.zeros(((n + 63) // 64 + 1) * 64, dtype=np.uint8)
        padded[:n] = np.asarray(self.bv, dtype=np.uint8)
        return np.packbits(padded, bitorder="little").view(np.uint64).copy()


class ProvingAssignment(ConstraintSystem):
    """prover.rs:57-162"""

    def __init__(self):
        self.a_aux_density, self.b_input_density, self.b_aux_density = _Density(), _Density(), _Density()
        self.a, self.b, self.c = [], [], []
        self.input_assignment, self.aux_assignment = [], []

    def alloc(self, f):
        self.aux_assignment.append(f() % Q)
        self.a_aux_density.add_element()
        self.b_aux_density.add_element()
        return Variable(AUX, len(self.aux_assignment) - 1)

    def alloc_input(self, f):
        self.input_assignment.append(f() % Q)
        self.b_input_density.add_element()
        return Variable(INPUT, len(self.input_assignment) - 1)

    def _eval(self, lc, input_density, aux_density):
        """prover.rs:19-55"""
        acc = 0
        for var, coeff in lc.terms:
            if coeff == 0:
                continue
            if var.kind == INPUT:
                tmp = self.input_assignment[var.idx]
                if input_density is not None:
                    input_density.inc(var.idx)
            else:
                tmp = self.aux_assignment[var.idx]
                if aux_density is not None:
                    aux_density.inc(var.idx)
            if coeff != 1:
                tmp = tmp * coeff % Q
            acc = (acc + tmp) % Q
        return acc

    def enforce(self, a, b, c):
        z = LinearCombination.zero()
        self.a.append(self._eval(a(z), None, self.a_aux_density))
        self.b.append(self._eval(b(z), self.b_input_density, self.b_aux_density))
        self.c.append(self._eval(c(z), None, None))


class Proof:
    """groth16/src/lib.rs:25-30: affine records (numpy uint64): a [12], b [24], c [12]."""

    def __init__(self, raw):
        self.a, self.b, self.c = raw[:12].copy(), raw[12:36].copy(), raw[36:48].copy()

    def write(self):
        """Proof::write (groth16/src/lib.rs:38-46): compressed A (48) | B (96) | C (48)"""
        raw = np.concatenate([self.a, self.b, self.c]).astype(np.uint64)
        out = np.zeros(192, dtype=np.uint8)
        _lib.load().bh_proof_write(raw.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        return out.tobytes()


    @classmethod
    def read(cls, worker, data):
        """Proof::read (groth16/src/lib.rs:47-99) of 192 bytes: the three points decompressed and checked on the device.
        Raises UnexpectedEof for a shorter input (read_exact), InvalidPoint / PointAtInfinity for a bad element."""
        data = bytes(data)
        if len(data) < 192:
            raise UnexpectedEof("failed to fill whole buffer")
        return read_proofs(worker, data[:192])[0]


def read_proofs(worker, data, return_status=False):
    """Proof::read over concatenated 192-byte proofs (bh_proofs_read).  Returns the list of proofs; the first bad proof in
    stream order raises InvalidPoint / PointAtInfinity with `.index` = its position.  return_status=True never raises
    for a bad proof: it returns (proofs, status) with one uint32 per proof (0 = good; the bits are documented at
    bh_proofs_read in include/bellman_hip.h) and None in place of every bad proof."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    if buf.size % 192:
        raise UnexpectedEof("failed to fill whole buffer")
    n = buf.size // 192
    out = np.zeros((n, 48), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    bad = ctypes.c_size_t(0)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.load().bh_proofs_read(worker.ctx, p(buf) if n else None, n, p(out) if n else None, p(status), ctypes.byref(bad))
    if return_status:
        if rc not in (C.BH_OK, C.BH_ERR_INVALID_POINT, C.BH_ERR_POINT_AT_INFINITY):
            check(rc, "proofs_read")
        return [Proof(out[i]) if status[i] == 0 else None for i in range(n)], status
    try:
        check(rc, "proofs_read")
    except IOError as e:
        e.index = bad.value
        raise
    return [Proof(out[i]) for i in range(n)]


class Parameters:
    """`&Parameters` as ParameterSource (groth16/src/lib.rs:435-473); query vectors live in HBM."""

    def __init__(self, worker, alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, h, l, a, b_g1, b_g2):
        lib = _lib.load()
        self.worker = worker
        arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2)]
        qs = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, w) for x, w in ((h, 12), (l, 12), (a, 12), (b_g1, 12), (b_g2, 24))]
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        h_ = ctypes.c_void_p()
        check(lib.bh_groth16_params_create(worker.ctx, *[p(x) for x in arrs], p(qs[0]), qs[0].shape[0], p(qs[1]),
                                           qs[1].shape[0], p(qs[2]), qs[2].shape[0], p(qs[3]), qs[3].shape[0],
                                           p(qs[4]), qs[4].shape[0], ctypes.byref(h_)), "Parameters")
        self._h = h_

    @classmethod
    def read(cls, worker, data, checked):
        """Parameters::read(reader, checked) (groth16/src/lib.rs:289-398): serialized CRS bytes ->
        device-resident parameters; decoding and validation run on the GPU.  Raises UnexpectedEof,
        InvalidPoint or PointAtInfinity - whichever the reference's sequential reader hits first."""
        lib = _lib.load()
        buf = np.frombuffer(data, dtype=np.uint8)   # bytes, bytearray or any buffer: no copy
        self = cls.__new__(cls)
        self.worker = worker
        h_ = ctypes.c_void_p()
        self._h = None
        check(lib.bh_groth16_params_read(worker.ctx, buf.ctypes.data_as(ctypes.c_void_p), buf.size, 1 if checked else 0,
                                         ctypes.byref(h_)), "Parameters.read")
        self._h = h_
        return self

    @classmethod
    def generate(cls, worker, r1cs, g1, g2, alpha, beta, gamma, delta, tau):
        """generate_parameters (groth16/src/generator.rs:163-510) on the device for the circuit whose
        matrices are `r1cs` (R1CS.from_circuit / from_demo).  g1, g2: affine Montgomery records (numpy
        uint64 [12] / [24]); alpha..tau: ints.  Raises UnexpectedIdentity (gamma or delta = 0),
        UnconstrainedVariable, PolynomialDegreeTooLarge."""
        lib = _lib.load()
        g1 = np.ascontiguousarray(g1, dtype=np.uint64)
        g2 = np.ascontiguousarray(g2, dtype=np.uint64)
        sc = fr_to_mont_array([alpha, beta, gamma, delta, tau])
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        self = cls.__new__(cls)
        self.worker, self._h = worker, None
        h_ = ctypes.c_void_p()
        check(lib.bh_groth16_generate(worker.ctx, r1cs._h, p(g1), p(g2), *[p(sc[i:i + 1]) for i in range(5)], ctypes.byref(h_)),
              "generate_parameters")
        self._h = h_
        return self

    @classmethod
    def from_powers_of_tau(cls, worker, r1cs, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2):
        """The parameters of generate(alpha, beta, 1, 1, tau) derived in the exponent from a powers-of-tau transcript
        (bh_groth16_generate_from_powers_of_tau): tau_g1 = [tau^i]G1 (at least 2m - 1 points), tau_g2 = [tau^i]G2,
        alpha_tau_g1, beta_tau_g1 (at least m each) as `Bases`, beta_g2 one affine G2 record ([24] uint64); m = the
        circuit's domain size.  Longer vectors are fine.  Validates nothing: read the transcript with
        Bases.read_uncompressed / read_compressed(checked=True).  Raises PolynomialDegreeTooLarge for a transcript that
        is too short, UnconstrainedVariable, AssertionError for a wrong-group handle.  `rescale_delta` then sets delta."""
        lib = _lib.load()
        b2 = np.ascontiguousarray(beta_g2, dtype=np.uint64).reshape(24)
        t = _PowersOfTau(*[x._h if x is not None else None for x in (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1)], b2.ctypes.data)
        self = cls.__new__(cls)
        self.worker, self._h = worker, None
        h_ = ctypes.c_void_p()
        check(lib.bh_groth16_generate_from_powers_of_tau(worker.ctx, r1cs._h, ctypes.byref(t), ctypes.byref(h_)),
              "Parameters.from_powers_of_tau")
        self._h = h_
        return self

    def rescale_delta(self, d):
        """New parameters with delta multiplied by d (an int mod q): delta_g1, delta_g2 *= d, h and l *= 1/d, the rest
        copied; `self` is unchanged.  d = 0 raises UnexpectedIdentity."""
        lib = _lib.load()
        sc = fr_to_mont_array([d % Q])
        out = Parameters.__new__(Parameters)
        out.worker, out._h = self.worker, None
        h_ = ctypes.c_void_p()
        check(lib.bh_groth16_params_rescale_delta(self._h, sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h_)),
              "Parameters.rescale_delta")
        out._h = h_
        return out

    def verify_step(self, after, seed=None, validate_points=True):
        """Is `after` this set with delta multiplied by some unknown d != 0 and nothing else changed - the receiver's check
        of one `rescale_delta` step (bh_groth16_params_verify_step): a, b_g1, b_g2 and the key are compared byte for byte on
        the device, h and l by one random linear combination per side, delta by pairings.  d = 1 passes.
        validate_points=True first puts `after`'s h, l, delta_g1 and delta_g2 through the curve and subgroup tests:
        InvalidPoint / PointAtInfinity with `.report` naming the vector (4 h, 5 l, 6 delta_g1, 7 delta_g2) and the index.
        `seed`: 32 bytes from which the coefficients are expanded; it MUST be drawn after `after` is fixed, from a CSPRNG -
        left None it comes from secrets.token_bytes.  Raises InvalidTranscript with `.report` (ParamsStepReport: the
        STEP_FAILED_* bits, bad_vector, bad_index); returns the report (failed == 0)."""
        import secrets

        from .errors import InvalidData, InvalidTranscript

        seed = secrets.token_bytes(32) if seed is None else bytes(seed)
        assert len(seed) == 32
        rep = ParamsStepReport()
        rc = _lib.load().bh_groth16_params_verify_step(self.worker.ctx, self._h, after._h, seed,
                                                       STEP_VALIDATE_POINTS if validate_points else 0, ctypes.byref(rep))
        if rc == C.BH_ERR_INVALID_TRANSCRIPT:
            raise InvalidTranscript(rep, "not a rescaling of delta alone")
        try:
            check(rc, "Parameters.verify_step")
        except InvalidData as e:
            e.report = rep
            raise
        return rep

    def write(self):
        """Parameters::write (groth16/src/lib.rs:258-287) -> bytes"""
        lib = _lib.load()
        n = ctypes.c_size_t()
        check(lib.bh_groth16_params_write(self._h, None, 0, ctypes.byref(n)), "Parameters.write")
        out = ctypes.create_string_buffer(n.value)
        check(lib.bh_groth16_params_write(self._h, ctypes.cast(out, ctypes.c_void_p), n.value, ctypes.byref(n)), "Parameters.write")
        return out.raw   # immutable, hashable bytes like the reference's Vec<u8> handed to a writer; write_into avoids the copy

    def serialized_len(self):
        """byte length of Parameters::write's output"""
        n = ctypes.c_size_t()
        check(_lib.load().bh_groth16_params_write(self._h, None, 0, ctypes.byref(n)), "Parameters.write")
        return n.value

    def write_into(self, buffer):
        """Parameters::write into a caller-provided writable buffer (bytearray, numpy uint8, mmap ...): no second copy of a
        CRS of half a gigabyte.  Returns the number of bytes written; the buffer must hold at least that many."""
        lib = _lib.load()
        n = ctypes.c_size_t()
        check(lib.bh_groth16_params_write(self._h, None, 0, ctypes.byref(n)), "Parameters.write")
        mv = memoryview(buffer).cast("B")
        if mv.readonly or len(mv) < n.value:
            raise ValueError("write_into needs a writable buffer of at least %d bytes" % n.value)
        view = (ctypes.c_ubyte * len(mv)).from_buffer(mv)
        check(lib.bh_groth16_params_write(self._h, ctypes.cast(view, ctypes.c_void_p), n.value, ctypes.byref(n)), "Parameters.write")
        del view
        return n.value

    def vk_ext(self):
        """gamma_g2 ([24] uint64) and ic ([n,12] uint64): the verifier-side key elements"""
        lib = _lib.load()
        n = ctypes.c_size_t()
        gamma = np.zeros(24, dtype=np.uint64)
        check(lib.bh_groth16_params_vk_ext(self._h, gamma.ctypes.data_as(ctypes.c_void_p), None, 0, ctypes.byref(n)), "vk_ext")
        ic = np.zeros((n.value, 12), dtype=np.uint64)
        check(lib.bh_groth16_params_vk_ext(self._h, None, ic.ctypes.data_as(ctypes.c_void_p), n.value, None), "vk_ext")
        return gamma, ic

    def query(self, which):
        """which in h, l, a, b_g1, b_g2 -> affine Montgomery records of that query, read back from HBM"""
        lib = _lib.load()
        idx = ("h", "l", "a", "b_g1", "b_g2").index(which)
        b, n = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib.bh_groth16_params_query(self._h, idx, ctypes.byref(b), ctypes.byref(n)), "Parameters.query")
        out = np.zeros((n.value, 24 if idx == 4 else 12), dtype=np.uint64)
        check(lib.bh_bases_download(self.worker.ctx, b, 0, n.value, out.ctypes.data_as(ctypes.c_void_p)), "Parameters.query")
        return out

    def bases(self, which):
        """the device-resident query itself as a (borrowed) Bases handle: get_h / get_l / get_a / get_b_g1 / get_b_g2 of
        ParameterSource (groth16/src/lib.rs:443-473) without the offset - for multiexps issued by the caller"""
        from .multiexp import Bases

        idx = ("h", "l", "a", "b_g1", "b_g2").index(which)
        b, n = ctypes.c_void_p(), ctypes.c_size_t()
        check(_lib.load().bh_groth16_params_query(self._h, idx, ctypes.byref(b), ctypes.byref(n)), "Parameters.bases")
        hb = Bases.__new__(Bases)
        hb.worker, hb.group, hb.n = self.worker, 2 if idx == 4 else 1, n.value
        hb._h = b
        hb.release = lambda: None   # owned by the parameters
        return hb

    def vk(self):
        """alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2 as affine Montgomery records"""
        outs = [np.zeros(w, dtype=np.uint64) for w in (12, 12, 24, 12, 24)]
        check(_lib.load().bh_groth16_params_vk(self._h, *[o.ctypes.data_as(ctypes.c_void_p) for o in outs]), "Parameters.vk")
        return outs

    def release(self):
        if self._h:
            _lib.load().bh_groth16_params_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def prove_assignment(prover, params, r, s, timings=None):
    """prover.rs:217-360 on a synthesised ProvingAssignment."""
    lib = _lib.load()
    a, b, c = (fr_to_mont_array(v) for v in (prover.a, prover.b, prover.c))
    ia, aa = fr_to_mont_array(prover.input_assignment), fr_to_mont_array(prover.aux_assignment)
    d1, d2, d3 = prover.a_aux_density.words(), prover.b_input_density.words(), prover.b_aux_density.words()
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_assignment(params._h, p(a), p(b), p(c), a.shape[0], p(ia), ia.shape[0], p(aa), aa.shape[0],
                                          p(d1), p(d2), p(d3), p(rs[0:1]), p(rs[1:2]), p(out), tm), "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


def create_proof(circuit, params, r, s, timings=None):
    """prover.rs:182-215: `circuit` is a callable circuit(cs) (the Circuit::synthesize body)."""
    prover = ProvingAssignment()
    prover.alloc_input(lambda: 1)
    circuit(prover)
    for i in range(len(prover.input_assignment)):
        prover.enforce(lambda lc, i=i: lc + Variable(INPUT, i), lambda lc: lc, lambda lc: lc)
    return prove_assignment(prover, params, r, s, timings)


def create_random_proof(circuit, params, rng=None, r1cs=None):
    """prover.rs:164-180: r and s drawn uniformly from Fr, then create_proof.  `rng` is any object with
    randrange (random.Random, random.SystemRandom); default: the operating system's CSPRNG.  With
    `r1cs` the constraint evaluation runs on the device (create_proof_r1cs)."""
    import random

    rng = rng or random.SystemRandom()
    r, s = rng.randrange(Q), rng.randrange(Q)
    if r1cs is not None:
        return create_proof_r1cs(circuit, r1cs, params, r, s)
    return create_proof(circuit, params, r, s)


def create_proof_demo(params, kind, size, seed, witness, constants, r, s, timings=None):
    """create_proof on one of the C++ demo circuits (groth16_capi.cpp): 0 = MiMCDemo, 1 = chain."""
    lib = _lib.load()
    wit = fr_to_mont_array(witness if isinstance(witness, np.ndarray) else list(witness))
    con = fr_to_mont_array(constants if isinstance(constants, np.ndarray) else list(constants)) if constants is not None \
        else np.zeros((1, 4), dtype=np.uint64)
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_demo(params._h, kind, size, seed, p(wit), p(con), p(rs[0:1]), p(rs[1:2]), p(out), tm),
          "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


# ---- constraint matrices resident in HBM -------------------------------------------


class ShapeAssembly(ConstraintSystem):
    """Structure-only ConstraintSystem: records the three matrices, never calls the value closures
    (what generator.rs:43-131 KeypairAssembly does when the CRS for the circuit is built)."""

    def __init__(self):
        self.num_inputs = self.num_aux = 0
        self.rows = ([], [], [])  # per matrix: list of rows, each a list of (kind, idx, coeff)

    def alloc(self, f):
        self.num_aux += 1
        return Variable(AUX, self.num_aux - 1)

    def alloc_input(self, f):
        self.num_inputs += 1
        return Variable(INPUT, self.num_inputs - 1)

    def enforce(self, a, b, c):
        z = LinearCombination.zero()
        for m, lc in enumerate((a(z), b(z), c(z))):
            self.rows[m].append([(v.kind, v.idx, k) for v, k in lc.terms if k != 0])  # prover.rs:31

    @staticmethod
    def capture(circuit):
        cs = ShapeAssembly()
        cs.alloc_input(lambda: 1)
        circuit(cs)
        for i in range(cs.num_inputs):  # prover.rs:208-215
            cs.enforce(lambda lc, i=i: lc + Variable(INPUT, i), lambda lc: lc, lambda lc: lc)
        return cs

    def csr(self):
        """-> (row_ptr, var, coeff_index) x3 as uint32 arrays, coefficient table (ints, [0] == 1)."""
        table, index = [1], {1: 0}
        out = []
        for rows in self.rows:
            row_ptr, var, coeff = [0], [], []
            for row in rows:
                for kind, idx, k in row:
                    if k not in index:
                        index[k] = len(table)
                        table.append(k)
                    var.append(idx if kind == INPUT else self.num_inputs + idx)
                    coeff.append(index[k])
                row_ptr.append(len(var))
            out.append(tuple(np.asarray(x, dtype=np.uint32) for x in (row_ptr, var, coeff)))
        return out, table


_PowersOfTau = _abi.STRUCTS["bh_powers_of_tau"]
_Csr = _abi.STRUCTS["bh_csr"]
SATISFIED = C.BH_R1CS_SATISFIED


def _stacked(vectors, n, k, what):
    """k witness vectors of n elements -> one [k, n, 4] uint64 Montgomery array (witness j at row j: the layout of the batch
    entry points).  A [k, n, 4] uint64 array is taken as it is; a vector of the wrong length is refused."""
    if isinstance(vectors, np.ndarray) and vectors.dtype == np.uint64 and vectors.ndim == 3 and vectors.shape[2] == 4:
        if vectors.shape[1] != n:
            check(C.BH_ERR_INVALID_ARG, "%s (the witnesses do not have the shape of the captured circuit)" % what)
        return np.ascontiguousarray(vectors)
    arrs = [fr_to_mont_array(x if isinstance(x, np.ndarray) else list(x)) for x in vectors]
    for j, a in enumerate(arrs):
        if a.shape[0] != n:
            check(C.BH_ERR_INVALID_ARG, "%s (witness %d does not have the shape of the captured circuit)" % (what, j))
    return np.ascontiguousarray(np.stack(arrs)) if n and k else np.zeros((k, 0, 4), dtype=np.uint64)


HINT_BITS, HINT_INV_OR_ZERO = C.BH_HINT_BITS, C.BH_HINT_INV_OR_ZERO
NO_VARIABLE = 0xFFFFFFFF


class BitsHint:
    """outs[j] = bit shift + j of the canonical integer of `lc` (a LinearCombination), as the field element 0 or 1: the
    advice a bit decomposition allocates (src/gadgets/num.rs to_bits_le, the result bits of an adder)."""

    def __init__(self, lc, outs, shift=0):
        self.kind, self.lc, self.outs, self.shift = HINT_BITS, lc, list(outs), shift


class InverseOrZeroHint:
    """out = 1 / lc, or 0 where lc is 0: the advice of an is-zero or a division gadget."""

    def __init__(self, lc, out):
        self.kind, self.lc, self.outs, self.shift = HINT_INV_OR_ZERO, lc, [out], 0


_WitnessHint = _abi.STRUCTS["bh_witness_hint"]
_SolverDesc = _abi.STRUCTS["bh_solver_desc"]


def solver_desc(supplied, hints):
    """bh_solver_desc from plain indices: supplied = variable indices (bh_csr.var numbering), hints = (kind, [(variable,
    coefficient)], [output variables], shift).  -> (the structure, the arrays it points into: keep them alive)."""
    table, index = [1], {1: 0}
    lc_var, lc_coeff, out_var = [], [], []
    recs = (_WitnessHint * max(len(hints), 1))()
    for h, (kind, lc, outs, shift) in enumerate(hints):
        b0, o0 = len(lc_var), len(out_var)
        for var, k in lc:
            k %= Q
            if k not in index:
                index[k] = len(table)
                table.append(k)
            lc_var.append(var)
            lc_coeff.append(index[k])
        out_var += list(outs)
        recs[h] = _WitnessHint(kind, b0, len(lc_var), o0, len(out_var), shift)
    keep = [np.asarray(x, dtype=np.uint32) for x in (list(supplied), lc_var, lc_coeff, out_var)] + [fr_to_mont_array(table), recs]
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    desc = _SolverDesc(ptr(keep[0]), keep[0].size, ctypes.addressof(recs) if hints else None, len(hints), ptr(keep[1]), ptr(keep[2]),
                       ptr(keep[3]), keep[4].ctypes.data, keep[4].shape[0])
    return desc, keep


class Solver:
    """A witness solver of one circuit (bh_r1cs_solver, R1CS.solver): completes witnesses on the GPU from the values of the
    supplied variables.  `.info`: supplied / defined / hinted variables, dependency levels, widest level."""

    def __init__(self, r1cs, handle):
        self.r1cs, self._h = r1cs, handle   # (the bh_r1cs must outlive the solver: the reference keeps it)
        counts = (ctypes.c_size_t * 5)()
        check(_lib.load().bh_r1cs_solver_info(self._h, counts), "R1CS.solver")
        self.info = dict(zip(("supplied", "defined", "hinted", "levels", "widest_level"), (int(x) for x in counts)))

    def solve_many(self, inputs_list, aux_list):
        """k witnesses as eval_many takes them, every vector at its full length (what stands in a slot that is not supplied
        does not matter) -> completed copies ([k, num_inputs, 4], [k, num_aux, 4]) uint64 Montgomery, the form
        prove_witness_batch and which_is_unsatisfied take without a conversion.  No constraint is checked."""
        lib = _lib.load()
        r = self.r1cs
        k = len(inputs_list)
        assert len(aux_list) == k, "one aux vector per witness"
        ins = _stacked(inputs_list, r.num_inputs, k, "Solver.solve_many").copy()
        auxs = _stacked(aux_list, r.num_aux, k, "Solver.solve_many").copy()
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        check(lib.bh_r1cs_solve_many(r.worker.ctx, self._h, p(ins), p(auxs), k), "Solver.solve_many")
        return ins, auxs

    def solve_many_dev(self, dev_witnesses, stream=None):
        """the same in place on DeviceWitnesses (bh_r1cs_solve_many_dev), enqueued on `stream`: what prove_witness_batch_dev
        reads afterwards without a host copy"""
        w = dev_witnesses
        check(_lib.load().bh_r1cs_solve_many_dev(self.r1cs.worker.ctx, self._h, w.inputs, w.in_stride, w.aux, w.aux_stride, w.k, stream),
              "Solver.solve_many_dev")

    def solve(self, input_assignment, aux_assignment):
        ins, auxs = self.solve_many([input_assignment], [aux_assignment])
        return ins[0], auxs[0]

    def release(self):
        if self._h:
            if getattr(self.r1cs.worker, "_ctx", None):   # as R1CS.release: the pool is gone with the Worker
                _lib.load().bh_r1cs_solver_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class R1CS:
    """The circuit's A/B/C matrices registered on the device (bh_r1cs)."""

    def __init__(self, worker, handle):
        self.worker, self._h = worker, handle
        lib = _lib.load()
        n = [ctypes.c_size_t() for _ in range(3)]
        check(lib.bh_r1cs_shape(self._h, *[ctypes.byref(x) for x in n]), "R1CS")
        self.num_inputs, self.num_aux, self.num_constraints = (x.value for x in n)

    @staticmethod
    def from_csr(worker, num_inputs, num_aux, matrices, coeff_table):
        lib = _lib.load()
        n_cons = len(matrices[0][0]) - 1
        keep = [tuple(np.ascontiguousarray(x, dtype=np.uint32) for x in m) for m in matrices]
        abc = (_Csr * 3)(*[_Csr(*[x.ctypes.data for x in m]) for m in keep])
        coeffs = fr_to_mont_array(list(coeff_table))
        h = ctypes.c_void_p()
        check(lib.bh_r1cs_create(worker.ctx, num_inputs, num_aux, n_cons, ctypes.byref(abc),
                                 coeffs.ctypes.data_as(ctypes.c_void_p), coeffs.shape[0], ctypes.byref(h)), "R1CS")
        return R1CS(worker, h)

    @staticmethod
    def from_circuit(worker, circuit):
        cs = ShapeAssembly.capture(circuit)
        matrices, table = cs.csr()
        return R1CS.from_csr(worker, cs.num_inputs, cs.num_aux, matrices, table)

    @staticmethod
    def from_demo(worker, kind, size, seed=0, constants=None):
        lib = _lib.load()
        con = fr_to_mont_array(list(constants)) if constants is not None else np.zeros((1, 4), dtype=np.uint64)
        h = ctypes.c_void_p()
        check(lib.bh_groth16_demo_r1cs(worker.ctx, kind, size, seed, con.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)), "R1CS")
        return R1CS(worker, h)

    def density(self, which):
        """which: 0 a_aux, 1 b_input, 2 b_aux -> (bool array, total)"""
        lib = _lib.load()
        host, total = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib.bh_r1cs_density(self._h, which, None, ctypes.byref(host), ctypes.byref(total)), "R1CS")
        n = self.num_inputs if which == 1 else self.num_aux
        nw = (n + 63) // 64
        words = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint64)), shape=(max(nw, 1),)).copy()
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        return bits, total.value

    def eval(self, input_assignment, aux_assignment):
        """a, b, c evaluations ([m,4] uint64 Montgomery, m = next power of two) - parity-test hook."""
        lib = _lib.load()
        ctx = self.worker.ctx
        log_m = 0
        while (1 << log_m) < self.num_constraints:
            log_m += 1
        m = 1 << log_m
        ia, aa = fr_to_mont_array(list(input_assignment)), fr_to_mont_array(list(aux_assignment))
        bufs = []
        for nbytes in (ia.nbytes + 32, aa.nbytes + 32, m * 32, m * 32, m * 32):
            d = ctypes.c_void_p()
            check(lib.bh_dev_alloc(ctx, nbytes, ctypes.byref(d)), "R1CS.eval")
            bufs.append(d)
        try:
            check(lib.bh_dev_upload(ctx, bufs[0], ia.ctypes.data_as(ctypes.c_void_p), ia.nbytes), "R1CS.eval")
            if aa.nbytes:
                check(lib.bh_dev_upload(ctx, bufs[1], aa.ctypes.data_as(ctypes.c_void_p), aa.nbytes), "R1CS.eval")
            check(lib.bh_r1cs_eval_dev(ctx, self._h, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], log_m, None), "R1CS.eval")
            outs = []
            for d in bufs[2:]:
                o = np.zeros((m, 4), dtype=np.uint64)
                check(lib.bh_dev_download(ctx, o.ctypes.data_as(ctypes.c_void_p), d, o.nbytes), "R1CS.eval")
                outs.append(o)
        finally:
            for d in bufs:
                lib.bh_dev_free(ctx, d)
        return outs

    def eval_many(self, inputs_list, aux_list):
        """a, b, c evaluations of k witnesses in one call (bh_r1cs_eval_many_dev): three [k, m, 4] uint64 Montgomery arrays,
        m = next power of two, row j exactly what eval returns for witness j - parity-test hook."""
        lib = _lib.load()
        ctx = self.worker.ctx
        k = len(inputs_list)
        assert len(aux_list) == k, "one aux vector per witness"
        log_m = 0
        while (1 << log_m) < self.num_constraints:
            log_m += 1
        m = 1 << log_m
        ins, auxs = _stacked(inputs_list, self.num_inputs, k, "R1CS.eval_many"), _stacked(aux_list, self.num_aux, k, "R1CS.eval_many")
        outs = [np.zeros((k, m, 4), dtype=np.uint64) for _ in range(3)]
        if k == 0:
            return outs
        bufs = []
        for nbytes in (ins.nbytes + 32, auxs.nbytes + 32, k * m * 32, k * m * 32, k * m * 32):
            d = ctypes.c_void_p()
            check(lib.bh_dev_alloc(ctx, nbytes, ctypes.byref(d)), "R1CS.eval_many")
            bufs.append(d)
        try:
            for d, a in ((bufs[0], ins), (bufs[1], auxs)):
                if a.nbytes:
                    check(lib.bh_dev_upload(ctx, d, a.ctypes.data_as(ctypes.c_void_p), a.nbytes), "R1CS.eval_many")
            check(lib.bh_r1cs_eval_many_dev(ctx, self._h, bufs[0], self.num_inputs * 32, bufs[1], self.num_aux * 32, k, bufs[2], bufs[3],
                                            bufs[4], m * 32, log_m, None), "R1CS.eval_many")
            for d, o in zip(bufs[2:], outs):
                check(lib.bh_dev_download(ctx, o.ctypes.data_as(ctypes.c_void_p), d, o.nbytes), "R1CS.eval_many")
        finally:
            for d in bufs:
                lib.bh_dev_free(ctx, d)
        return outs

    def which_is_unsatisfied(self, inputs_list, aux_list):
        """TestConstraintSystem::which_is_unsatisfied (src/gadgets/test/mod.rs:254-272) for k witnesses in one GPU pass
        (bh_r1cs_check_many): entry j is the index of the first constraint witness j = (inputs_list[j], aux_list[j]) does
        not satisfy, or None.  Witnesses as prove_witness_batch takes them."""
        lib = _lib.load()
        k = len(inputs_list)
        assert len(aux_list) == k, "one aux vector per witness"
        ins = _stacked(inputs_list, self.num_inputs, k, "R1CS.which_is_unsatisfied")
        auxs = _stacked(aux_list, self.num_aux, k, "R1CS.which_is_unsatisfied")
        if k == 0:
            return []
        bad = np.zeros(k, dtype=np.uint32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        check(lib.bh_r1cs_check_many(self.worker.ctx, self._h, p(ins), p(auxs), k, p(bad)), "R1CS.which_is_unsatisfied")
        return [None if int(b) == SATISFIED else int(b) for b in bad]

    def is_satisfied(self, input_assignment, aux_assignment):
        """TestConstraintSystem::is_satisfied for one witness"""
        return self.which_is_unsatisfied([input_assignment], [aux_assignment])[0] is None

    def solver(self, supplied, hints=()):
        """A Solver for this circuit: `supplied` = the Variables whose values the caller provides (what the circuit takes
        from outside), `hints` = BitsHint / InverseOrZeroHint for advice values; every other variable must be the new
        variable of an `alloc` + `enforce(a, b, c)` pair, alone in c (include/bellman_hip.h has the rule).  ValueError names
        the first Variable that is not determined that way, or that a hint may not write."""
        lib = _lib.load()
        idx = lambda v: v.idx if v.kind == INPUT else self.num_inputs + v.idx  # noqa: E731
        desc, keep = solver_desc([idx(v) for v in supplied],
                                 [(h.kind, [(idx(v), k) for v, k in h.lc.terms], [idx(v) for v in h.outs], h.shift) for h in hints])
        bad, h = ctypes.c_uint32(NO_VARIABLE), ctypes.c_void_p()
        rc = lib.bh_r1cs_solver_create(self.worker.ctx, self._h, ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(h))
        del keep
        if rc == C.BH_ERR_INVALID_ARG and bad.value != NO_VARIABLE:
            v = bad.value
            name = "Variable(INPUT, %d)" % v if v < self.num_inputs else "Variable(AUX, %d)" % (v - self.num_inputs)
            raise ValueError("R1CS.solver: %s is not determined by the supplied variables, the hints and the constraints in "
                             "order, or is written by a hint that may not write it" % name)
        check(rc, "R1CS.solver")
        return Solver(self, h)

    def eval_transposed_points(self, group, matrix, lagrange, accumulate_into=None, stream=None):
        """The raw group-valued product (bh_r1cs_eval_transposed_points_dev): out[v] = sum_j coeff * lagrange[j] over the
        constraints j that use variable v in `matrix` (0 A, 1 B, 2 C).  lagrange: at least num_constraints affine records
        ([n, 12|24] uint64); accumulate_into: records the product is added to.  Returns [num_inputs + num_aux, 12|24]."""
        lib = _lib.load()
        ctx = self.worker.ctx
        words = 12 if group == 1 else 24
        lag = np.ascontiguousarray(lagrange, dtype=np.uint64).reshape(-1, words)
        if lag.shape[0] < self.num_constraints:
            raise AssertionError("eval_transposed_points: fewer Lagrange points than constraints")
        n_vars = self.num_inputs + self.num_aux
        out = np.zeros((n_vars, words), dtype=np.uint64)
        if accumulate_into is not None:
            out[:] = np.ascontiguousarray(accumulate_into, dtype=np.uint64).reshape(n_vars, words)
        bufs = []
        for nbytes in (lag.nbytes + 16, out.nbytes + 16):
            d = ctypes.c_void_p()
            check(lib.bh_dev_alloc(ctx, nbytes, ctypes.byref(d)), "R1CS.eval_transposed_points")
            bufs.append(d)
        try:
            if lag.nbytes:
                check(lib.bh_dev_upload(ctx, bufs[0], lag.ctypes.data_as(ctypes.c_void_p), lag.nbytes), "R1CS.eval_transposed_points")
            if accumulate_into is not None and out.nbytes:
                check(lib.bh_dev_upload(ctx, bufs[1], out.ctypes.data_as(ctypes.c_void_p), out.nbytes), "R1CS.eval_transposed_points")
            check(lib.bh_r1cs_eval_transposed_points_dev(ctx, self._h, group, matrix, bufs[0], bufs[1],
                                                         1 if accumulate_into is not None else 0, stream),
                  "R1CS.eval_transposed_points")
            if stream is not None:
                check(lib.bh_stream_synchronize(ctx, stream), "R1CS.eval_transposed_points")
            if out.nbytes:   # bh_dev_download runs on the context stream, after the product when stream is None
                check(lib.bh_dev_download(ctx, out.ctypes.data_as(ctypes.c_void_p), bufs[1], out.nbytes), "R1CS.eval_transposed_points")
        finally:
            for d in bufs:
                lib.bh_dev_free(ctx, d)
        return out

    def release(self):
        if self._h:
            # the matrices live in the context's pool: once the Worker is closed the context (and that memory) is gone,
            # and the handle must not reach back into it (a finaliser that runs after the Worker's, e.g. at interpreter exit)
            if getattr(self.worker, "_ctx", None):
                _lib.load().bh_r1cs_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class WitnessAssignment(ConstraintSystem):
    """prover.rs:57-162 reduced to witness generation (enforce is a no-op)."""

    def __init__(self):
        self.input_assignment, self.aux_assignment = [], []

    def alloc(self, f):
        self.aux_assignment.append(f() % Q)
        return Variable(AUX, len(self.aux_assignment) - 1)

    def alloc_input(self, f):
        self.input_assignment.append(f() % Q)
        return Variable(INPUT, len(self.input_assignment) - 1)

    def enforce(self, a, b, c):
        pass


def prove_witness(r1cs, params, input_assignment, aux_assignment, r, s, timings=None):
    lib = _lib.load()
    ia, aa = fr_to_mont_array(list(input_assignment)), fr_to_mont_array(list(aux_assignment))
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_witness(params._h, r1cs._h, p(ia), ia.shape[0], p(aa), aa.shape[0], p(rs[0:1]), p(rs[1:2]),
                                       p(out), tm), "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


def prove_witness_batch(r1cs, params, inputs_list, aux_list, rs, ss, timings=None, _workspace_budget=None, _mode=None, _codes=None,
                        check=False, _first_unsatisfied=None, solver=None):
    """k proofs of ONE circuit in one call (bh_groth16_prove_witness_batch): witness j = (inputs_list[j], aux_list[j]),
    blinding (rs[j], ss[j]) -> [Proof], each exactly what prove_witness returns for that witness.  inputs_list / aux_list:
    lists of integer lists or [n, 4] Montgomery arrays, or one [k, n, 4] uint64 array each (no copy is made then).  A witness of the wrong
    shape is refused for the whole call before anything runs, as the single call refuses it; otherwise the error the
    first failing proof would raise is raised.  (_workspace_budget: the test library's twin of the call, which takes the
    grouped path - many-jobs over groups of witnesses that fit that many bytes of h-block workspace, 0 = the default 1 GiB -
    instead of keeping the proofs in flight.  _mode: the twin that takes the path of groth16.hpp's BATCH_* modes - 1 the
    grouped path, 2 the grouped path with a batched h block (bh_h_poly_fr_many_dev_on), groups by 4 * g * m * 32 bytes.
    3 the same with the group's constraint evaluations as ONE bh_r1cs_eval_many_dev and one upload per vector kind
    (bh_test_groth16_prove_witness_batch_he).
    _codes: a list that receives the per-proof return codes instead of the first failing one being raised.)
    check=True: every witness is first checked against the circuit's constraints on the GPU
    (bh_groth16_prove_witness_batch_checked); a witness with an unsatisfied constraint gets no proof - errors.Unsatisfiable
    (`.index` = the constraint) is raised for the first one, or with _codes its code is 11 and its slot None.
    _first_unsatisfied: a list that receives, per witness, the first unsatisfied constraint or None.
    solver: a Solver of r1cs (R1CS.solver) - the witnesses are completed through it first (Solver.solve_many: only the
    supplied variables' slots need to hold values); with check=True the check then judges the completed witnesses."""
    lib = _lib.load()
    check_witnesses, check = check, _check_rc
    k = len(inputs_list)
    assert len(aux_list) == k and len(rs) == k and len(ss) == k, "one aux vector and one (r, s) per witness"
    assert not check_witnesses or (_mode is None and _workspace_budget is None), "the checked entry point has no test twin"
    ins = _stacked(inputs_list, r1cs.num_inputs, k, "create_proof")
    auxs = _stacked(aux_list, r1cs.num_aux, k, "create_proof")
    if solver is not None and k:
        ins, auxs = solver.solve_many(ins, auxs)
    if k == 0:
        if _first_unsatisfied is not None:
            _first_unsatisfied[:] = []
        return []
    rr, sv = fr_to_mont_array(list(rs)), fr_to_mont_array(list(ss))
    out = np.zeros((k, 48), dtype=np.uint64)
    rcs = np.zeros(k, dtype=np.int32)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    first_bad = np.full(k, SATISFIED, dtype=np.uint32)
    if check_witnesses:
        rc = lib.bh_groth16_prove_witness_batch_checked(params._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k, p(rr),
                                                        p(sv), p(out), p(rcs), p(first_bad), tm)
    elif _mode == 3:   # BATCH_GROUPED_HE has a hook of its own: the mode hook keeps refusing what it refused before
        rc = lib.bh_test_groth16_prove_witness_batch_he(params._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k, p(rr), p(sv),
                                                        p(out), p(rcs), _workspace_budget or 0, tm)
    elif _mode is not None:
        rc = lib.bh_test_groth16_prove_witness_batch_mode(params._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k,
                                                          p(rr), p(sv), p(out), p(rcs), _workspace_budget or 0, _mode, tm)
    elif _workspace_budget is None:
        rc = lib.bh_groth16_prove_witness_batch(params._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k, p(rr), p(sv),
                                                p(out), p(rcs), tm)
    else:
        rc = lib.bh_test_groth16_prove_witness_batch_budget(params._h, r1cs._h, p(ins), r1cs.num_inputs, p(auxs), r1cs.num_aux, k,
                                                            p(rr), p(sv), p(out), p(rcs), _workspace_budget, tm)
    check(rc, "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    if _first_unsatisfied is not None:
        _first_unsatisfied[:] = [None if int(b) == SATISFIED else int(b) for b in first_bad]
    if _codes is not None:
        _codes[:] = [int(c) for c in rcs]
        return [Proof(out[j].copy()) if rcs[j] == 0 else None for j in range(k)]
    for j in range(k):
        if int(rcs[j]) == C.BH_ERR_UNSATISFIABLE:
            raise Unsatisfiable(int(first_bad[j]))
        check(int(rcs[j]), "create_proof")
    return [Proof(out[j].copy()) for j in range(k)]


PROVE_CHECK, PROVE_FINISH_DEVICE, PROVE_FINISH_HOST = C.BH_PROVE_CHECK, C.BH_PROVE_FINISH_DEVICE, C.BH_PROVE_FINISH_HOST


class DeviceWitnesses:
    """k witnesses of one circuit in device memory, as bh_r1cs_solve_many_dev / bh_r1cs_check_many_dev /
    bh_groth16_prove_witness_batch_dev take them: witness j's vectors at inputs + j * in_stride and aux + j * aux_stride
    (bytes).  Owns its two buffers (release)."""

    def __init__(self, worker, inputs, in_stride, aux, aux_stride, k, n_inputs, n_aux):
        self.worker, self.inputs, self.in_stride, self.aux, self.aux_stride = worker, inputs, in_stride, aux, aux_stride
        self.k, self.n_inputs, self.n_aux = k, n_inputs, n_aux

    @classmethod
    def from_host(cls, worker, ins, auxs, stride_extra=0):
        """ins / auxs: [k, n, 4] uint64 Montgomery arrays; stride_extra: bytes of padding behind every vector (a multiple of
        32), filled with a pattern so that a test can see it unchanged"""
        lib = _lib.load()
        ins, auxs = np.ascontiguousarray(ins, dtype=np.uint64), np.ascontiguousarray(auxs, dtype=np.uint64)
        k = ins.shape[0]
        assert auxs.shape[0] == k and stride_extra % 32 == 0
        bufs = []
        for v in (ins, auxs):
            n = v.shape[1]
            padded = np.full((k, n * 4 + stride_extra // 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :n * 4] = v.reshape(k, n * 4)
            d = ctypes.c_void_p()
            check(lib.bh_dev_alloc(worker.ctx, max(padded.nbytes, 32), ctypes.byref(d)), "DeviceWitnesses")
            if padded.nbytes:
                check(lib.bh_dev_upload(worker.ctx, d, padded.ctypes.data_as(ctypes.c_void_p), padded.nbytes), "DeviceWitnesses")
            bufs.append(d)
        return cls(worker, bufs[0], ins.shape[1] * 32 + stride_extra, bufs[1], auxs.shape[1] * 32 + stride_extra, k,
                   ins.shape[1], auxs.shape[1])

    def download_raw(self):
        """the two buffers as they are, padding included: ([k, in_stride / 8], [k, aux_stride / 8]) uint64"""
        lib = _lib.load()
        out = []
        for d, stride in ((self.inputs, self.in_stride), (self.aux, self.aux_stride)):
            a = np.zeros((self.k, stride // 8), dtype=np.uint64)
            if a.nbytes:
                check(lib.bh_dev_download(self.worker.ctx, a.ctypes.data_as(ctypes.c_void_p), d, a.nbytes), "DeviceWitnesses")
            out.append(a)
        return out

    def download(self):
        """([k, n_inputs, 4], [k, n_aux, 4]) uint64 Montgomery"""
        i, a = self.download_raw()
        return (np.ascontiguousarray(i[:, :self.n_inputs * 4]).reshape(self.k, self.n_inputs, 4),
                np.ascontiguousarray(a[:, :self.n_aux * 4]).reshape(self.k, self.n_aux, 4))

    def release(self):
        if self.inputs is not None:
            if getattr(self.worker, "_ctx", None):
                for d in (self.inputs, self.aux):
                    _lib.load().bh_dev_free(self.worker.ctx, d)
            self.inputs = self.aux = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def prove_witness_batch_dev(r1cs, params, dev_witnesses, rs, ss, check=False, solver=None, finish=None, _mode=None, _codes=None,
                            _first_unsatisfied=None, timings=None, stream=None, _workspace_budget=None):
    """prove_witness_batch over witnesses that are in device memory already (bh_groth16_prove_witness_batch_dev): nothing
    is uploaded, the buffers are read in place.  check / _codes / _first_unsatisfied / the errors raised: as
    prove_witness_batch.  finish: None (the measured rule), "host" or "device" (the proofs' tails by
    bh_proof_finish_dev's kernels).  solver: Solver.solve_many_dev on the buffers first, then the prover behind it on the
    same stream - no host copy of a solved witness exists.  _mode (0 or 3) / _workspace_budget: the test library's twin
    of the call (bh_test_groth16_prove_witness_batch_dev_mode) - 3 is the grouped path of groth16.hpp's BATCH_GROUPED_HE over
    runs of consecutive proved witnesses that fit the budget."""
    lib = _lib.load()
    check_witnesses, check = check, _check_rc
    w = dev_witnesses
    k = w.k
    if len(rs) != k or len(ss) != k:
        raise ValueError("one (r, s) per witness")
    if (w.n_inputs, w.n_aux) != (r1cs.num_inputs, r1cs.num_aux):
        raise ValueError("witnesses of another circuit")
    finish_bits = {None: 0, "host": PROVE_FINISH_HOST, "device": PROVE_FINISH_DEVICE}
    if finish not in finish_bits:
        raise ValueError("finish: None, 'host' or 'device'")
    flags = (PROVE_CHECK if check_witnesses else 0) | finish_bits[finish]
    if solver is not None and k:
        solver.solve_many_dev(w, stream)
    rr, sv = fr_to_mont_array(list(rs)), fr_to_mont_array(list(ss))
    out = np.zeros((max(k, 1), 48), dtype=np.uint64)
    rcs = np.zeros(max(k, 1), dtype=np.int32)
    first_bad = np.full(max(k, 1), SATISFIED, dtype=np.uint32)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if _mode is None and _workspace_budget is None:
        rc = lib.bh_groth16_prove_witness_batch_dev(params._h, r1cs._h, w.inputs, w.in_stride, w.aux, w.aux_stride, k, p(rr), p(sv), flags,
                                                    stream, p(out), p(rcs), p(first_bad), tm)
    else:
        rc = lib.bh_test_groth16_prove_witness_batch_dev_mode(params._h, r1cs._h, w.inputs, w.in_stride, w.aux, w.aux_stride, k, p(rr),
                                                              p(sv), flags, stream, p(out), p(rcs), p(first_bad), tm,
                                                              _workspace_budget or 0, _mode or 0)
    check(rc, "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    if _first_unsatisfied is not None:
        _first_unsatisfied[:] = [None if int(b) == SATISFIED else int(b) for b in first_bad[:k]]
    if _codes is not None:
        _codes[:] = [int(c) for c in rcs[:k]]
        return [Proof(out[j].copy()) if rcs[j] == 0 else None for j in range(k)]
    for j in range(k):
        if int(rcs[j]) == C.BH_ERR_UNSATISFIABLE:
            raise Unsatisfiable(int(first_bad[j]))
        check(int(rcs[j]), "create_proof")
    return [Proof(out[j].copy()) for j in range(k)]


def create_proof_r1cs(circuit, r1cs, params, r, s, timings=None):
    """create_proof with the constraint evaluation on the device: only `circuit`'s value closures run here."""
    w = WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return prove_witness(r1cs, params, w.input_assignment, w.aux_assignment, r, s, timings)


def create_proof_demo_r1cs(params, r1cs, kind, size, seed, witness, constants, r, s, timings=None):
    lib = _lib.load()
    wit = fr_to_mont_array(witness if isinstance(witness, np.ndarray) else list(witness))
    con = fr_to_mont_array(constants if isinstance(constants, np.ndarray) else list(constants)) if constants is not None \
        else np.zeros((1, 4), dtype=np.uint64)
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_demo_r1cs(params._h, r1cs._h, kind, size, seed, p(wit), p(con), p(rs[0:1]), p(rs[1:2]),
                                         p(out), tm), "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


# ---- one proof over several GPUs ------------------------------------------------------
SUMS_WORDS = C.BH_MSM_SUMS_BYTES // 8


def prove_witness_part(r1cs, params, input_assignment, aux_assignment, part, parts, timings=None):
    """The eight multiexp results of create_proof over part `part` of `parts` of the scalar indices
    -> uint64[120] (a_inputs, a_aux, b_g1_inputs, b_g1_aux | b_g2_inputs, b_g2_aux | h, l)."""
    lib = _lib.load()
    ia, aa = fr_to_mont_array(list(input_assignment)), fr_to_mont_array(list(aux_assignment))
    out = np.zeros(SUMS_WORDS, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_witness_part(params._h, r1cs._h, p(ia), ia.shape[0], p(aa), aa.shape[0], part, parts, p(out), tm),
          "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return out


def prove_demo_part(params, r1cs, kind, size, seed, witness, constants, part, parts, timings=None):
    lib = _lib.load()
    wit = fr_to_mont_array(list(witness))
    con = fr_to_mont_array(list(constants)) if constants is not None else np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros(SUMS_WORDS, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_demo_r1cs_part(params._h, r1cs._h, kind, size, seed, p(wit), p(con), part, parts, p(out), tm),
          "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return out


def sums_add(acc, other):
    """slot-wise group addition of two multiexp-result records (host code)"""
    acc = np.ascontiguousarray(acc, dtype=np.uint64).copy()
    other = np.ascontiguousarray(other, dtype=np.uint64)
    _lib.load().bh_groth16_sums_add(acc.ctypes.data_as(ctypes.c_void_p), other.ctypes.data_as(ctypes.c_void_p))
    return acc


def assemble(params, sums, r, s):
    """prover.rs:326-360 from the (summed) multiexp results"""
    rs = fr_to_mont_array([r, s])
    sums = np.ascontiguousarray(sums, dtype=np.uint64)
    out = np.zeros(48, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(_lib.load().bh_groth16_assemble(params._h, p(sums), p(rs[0:1]), p(rs[1:2]), p(out)), "create_proof")
    return Proof(out)


def assemble_many(params, sums_list, rs, ss, _codes=None):
    """k proofs from k sets of (summed) multiexp results in one device call (bh_groth16_assemble_many): proof j is exactly
    assemble(params, sums_list[j], rs[j], ss[j]).  Raises what the first failing proof would (an identity delta:
    UnexpectedIdentity); with _codes (a list) the per-proof codes are appended instead and failed slots are all zero."""
    k = len(sums_list)
    if len(rs) != k or len(ss) != k:
        raise ValueError("one (r, s) per set of sums")
    out = np.zeros((k, 48), dtype=np.uint64)
    if not k:
        return []
    sums = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.uint64).reshape(SUMS_WORDS) for x in sums_list]))
    r, s = fr_to_mont_array(list(rs)), fr_to_mont_array(list(ss))
    rcs = np.zeros(k, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(_lib.load().bh_groth16_assemble_many(params._h, p(sums), p(r), p(s), k, p(out), p(rcs)), "create_proof")
    if _codes is not None:
        _codes.extend(int(c) for c in rcs)
    else:
        for c in rcs:
            check(int(c), "create_proof")
    return [Proof(out[j].copy()) for j in range(k)]


# ---- the reference's call sites as the Rust shim issues them (shim/patches, csrc/groth16_callsites.cpp) ----------


def demo_assignment(kind, size, seed, witness, constants=None):
    """The ProvingAssignment create_proof synthesises for a C++ demo circuit (prover.rs:182-215), as numpy arrays:
    dict(a, b, c, input_assignment, aux_assignment: [n,4] uint64 Montgomery; a_aux_density, b_input_density,
    b_aux_density: LSB0 uint64 words).  Host only (test hook)."""
    lib = _lib.load()
    wit = fr_to_mont_array(witness if isinstance(witness, np.ndarray) else list(witness))
    con = fr_to_mont_array(constants if isinstance(constants, np.ndarray) else list(constants)) if constants is not None \
        else np.zeros((1, 4), dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    counts = (ctypes.c_size_t * 3)()
    check(lib.bh_test_demo_assignment(kind, size, seed, p(wit), p(con), counts, None, None, None, None, None, None, None, None))
    nc, ni, na = counts[0], counts[1], counts[2]
    out = dict(a=np.zeros((nc, 4), np.uint64), b=np.zeros((nc, 4), np.uint64), c=np.zeros((nc, 4), np.uint64),
               input_assignment=np.zeros((ni, 4), np.uint64), aux_assignment=np.zeros((na, 4), np.uint64),
               a_aux_density=np.zeros((na + 63) // 64 + 1, np.uint64), b_input_density=np.zeros((ni + 63) // 64 + 1, np.uint64),
               b_aux_density=np.zeros((na + 63) // 64 + 1, np.uint64))
    check(lib.bh_test_demo_assignment(kind, size, seed, p(wit), p(con), counts, p(out["a"]), p(out["b"]), p(out["c"]),
                                      p(out["input_assignment"]), p(out["aux_assignment"]), p(out["a_aux_density"]),
                                      p(out["b_input_density"]), p(out["b_aux_density"])))
    return out


def prove_assignment_arrays(params, asg, r, s, timings=None):
    """bh_groth16_prove_assignment on the arrays of demo_assignment (already Montgomery)."""
    lib = _lib.load()
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 4)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib.bh_groth16_prove_assignment(params._h, p(asg["a"]), p(asg["b"]), p(asg["c"]), asg["a"].shape[0],
                                          p(asg["input_assignment"]), asg["input_assignment"].shape[0], p(asg["aux_assignment"]),
                                          asg["aux_assignment"].shape[0], p(asg["a_aux_density"]), p(asg["b_input_density"]),
                                          p(asg["b_aux_density"]), p(rs[0:1]), p(rs[1:2]), p(out), tm), "create_proof")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


def prove_via_call_sites(params, asg, r, s, patched_prover, timings=None):
    """The h block + eight multiexps issued as bellman's create_proof issues them through the Rust shim:
    patched_prover=True  - groth16/src/prover.rs patched (scalars registered once, h block in one device call);
    patched_prover=False - only multiexp.rs / domain.rs patched (7 host FFT round trips, host pointwise passes, serial
                           Fr -> Exponent, 8 multiexps each uploading its scalars);
    patched_prover="resident" - the same patch level with the EvaluationDomain's vector kept in HBM between its calls,
                           `Exponent::from` deferred (no conversion on the host) and each shared exponent vector
                           uploaded once (csrc/groth16_callsites.cpp mode 2).
    timings: [issue + waits, total] host ms."""
    lib = _lib.load()
    rs = fr_to_mont_array([r, s])
    out = np.zeros(48, dtype=np.uint64)
    tm = (ctypes.c_float * 2)()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    mode = 2 if patched_prover == "resident" else 1 if patched_prover else 0
    check(lib.bh_test_groth16_prove_via_call_sites(params._h, mode, p(asg["a"]), p(asg["b"]), p(asg["c"]),
                                                   asg["a"].shape[0], p(asg["input_assignment"]), asg["input_assignment"].shape[0],
                                                   p(asg["aux_assignment"]), asg["aux_assignment"].shape[0], p(asg["a_aux_density"]),
                                                   p(asg["b_input_density"]), p(asg["b_aux_density"]), p(rs[0:1]), p(rs[1:2]), p(out), tm),
          "create_proof (call sites)")
    if timings is not None:
        timings[:] = list(tm)
    return Proof(out)


def create_proof_demo_async(params, r1cs, kind, size, seed, witness, constants, r, s):
    """bh_groth16_prove_demo_async: synthesis of the C++ demo circuit on this thread, the device part on a helper thread.
    Returns wait(timings=None) -> Proof.  r1cs=None: host synthesis as in the reference."""
    lib = _lib.load()
    wit = fr_to_mont_array(witness if isinstance(witness, np.ndarray) else list(witness))
    con = fr_to_mont_array(constants if isinstance(constants, np.ndarray) else list(constants)) if constants is not None \
        else np.zeros((1, 4), dtype=np.uint64)
    rs = fr_to_mont_array([r, s])
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    job = ctypes.c_void_p()
    check(lib.bh_groth16_prove_demo_async(params._h, None if r1cs is None else r1cs._h, kind, size, seed, p(wit), p(con),
                                          p(rs[0:1]), p(rs[1:2]), ctypes.byref(job)), "create_proof (async)")

    def wait(timings=None):
        out = np.zeros(48, dtype=np.uint64)
        tm = (ctypes.c_float * 4)()
        check(lib.bh_groth16_proof_wait(job, p(out), tm), "create_proof (async wait)")
        if timings is not None:
            timings[:] = list(tm)
        return Proof(out)

    return wait


def _proof_waiter(lib, job, keep):
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def wait(timings=None):
        _alive = keep  # noqa: F841  (the arrays the device part reads in place stay referenced until the wait)
        out = np.zeros(48, dtype=np.uint64)
        tm = (ctypes.c_float * 4)()
        check(lib.bh_groth16_proof_wait(job, p(out), tm), "create_proof (async wait)")
        if timings is not None:
            timings[:] = list(tm)
        return Proof(out)

    return wait


def prove_assignment_arrays_async(params, asg, r, s):
    """bh_groth16_prove_assignment_async on the arrays of demo_assignment: the device part of create_proof
    (prover.rs:217-360) on a helper thread; the arrays are read in place until the returned wait() has been called."""
    lib = _lib.load()
    rs = fr_to_mont_array([r, s])
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    job = ctypes.c_void_p()
    check(lib.bh_groth16_prove_assignment_async(params._h, p(asg["a"]), p(asg["b"]), p(asg["c"]), asg["a"].shape[0],
                                                p(asg["input_assignment"]), asg["input_assignment"].shape[0],
                                                p(asg["aux_assignment"]), asg["aux_assignment"].shape[0], p(asg["a_aux_density"]),
                                                p(asg["b_input_density"]), p(asg["b_aux_density"]), p(rs[0:1]), p(rs[1:2]),
                                                ctypes.byref(job)), "create_proof (async)")
    return _proof_waiter(lib, job, (asg, rs))


def prove_witness_async(r1cs, params, input_assignment, aux_assignment, r, s):
    """bh_groth16_prove_witness_async: the witness vectors (Montgomery [n,4] uint64 arrays, or lists of ints) are copied
    before this returns; the device part runs on a helper thread.  Returns wait(timings=None) -> Proof."""
    lib = _lib.load()
    ia = input_assignment if isinstance(input_assignment, np.ndarray) else fr_to_mont_array(list(input_assignment))
    aa = aux_assignment if isinstance(aux_assignment, np.ndarray) else fr_to_mont_array(list(aux_assignment))
    rs = fr_to_mont_array([r, s])
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    job = ctypes.c_void_p()
    check(lib.bh_groth16_prove_witness_async(params._h, r1cs._h, p(ia), ia.shape[0], p(aa), aa.shape[0], p(rs[0:1]), p(rs[1:2]),
                                             ctypes.byref(job)), "create_proof (async)")
    return _proof_waiter(lib, job, (r1cs,))
