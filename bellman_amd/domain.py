"""`EvaluationDomain` mirror (reference: src/domain.rs:21-190) for the `Scalar<Fr>` instantiation, and
`PointEvaluationDomain` for the `Point<G>` one (:192-229).

Coefficients are numpy uint64 [m,4] Montgomery-form Fr (the bytes of Rust `bls12_381::Scalar`s), or [m,12] / [m,24]
affine G1 / G2 records (Montgomery coordinates, all-zero = identity).  Every operation runs on the GPU through the C ABI;
the vector lives in HBM between calls."""

import ctypes

import numpy as np

from . import _lib
from ._abi import C
from .errors import PolynomialDegreeTooLarge, check

FR_S = 32  # 2-adicity of BLS12-381 Fr (ff::PrimeField::S)


class EvaluationDomain:
    def __init__(self, worker, dev, m, exp):
        self.worker, self._dev, self.m, self.exp = worker, dev, m, exp
        self._lib = _lib.load()

    @classmethod
    def from_coeffs(cls, worker, coeffs):
        """domain.rs:47-79: pad to m = next power of two >= len with zeros; exp >= S errors."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        m, exp = 1, 0
        while m < coeffs.shape[0]:
            m *= 2
            exp += 1
            if exp >= FR_S:
                raise PolynomialDegreeTooLarge()
        if coeffs.shape[0] == m:
            padded = coeffs   # already a full domain: no second host copy (8 GiB at 2^28)
        else:
            padded = np.zeros((m, 4), dtype=np.uint64)
            padded[: coeffs.shape[0]] = coeffs
        dev = worker.alloc(m * 32)
        worker.upload(dev, padded)
        return cls(worker, dev, m, exp)

    def __len__(self):
        return self.m

    def into_coeffs(self):
        out = np.empty((self.m, 4), dtype=np.uint64)
        self.worker.download(out, self._dev)
        self.worker.free(self._dev)
        self._dev = None
        return out

    def as_ref(self):
        out = np.empty((self.m, 4), dtype=np.uint64)
        self.worker.download(out, self._dev)
        return out

    def _fft(self, mode):
        check(self._lib.bh_fft_fr_dev(self.worker.ctx, self._dev, self.exp, mode, None), "fft")
        self.worker.synchronize()

    def fft(self, worker=None):
        self._fft(C.BH_FFT)

    def ifft(self, worker=None):
        self._fft(C.BH_IFFT)

    def coset_fft(self, worker=None):
        self._fft(C.BH_COSET_FFT)

    def icoset_fft(self, worker=None):
        self._fft(C.BH_ICOSET_FFT)

    def distribute_powers(self, worker, g_mont):
        g = np.ascontiguousarray(g_mont, dtype=np.uint64).reshape(4)
        check(self._lib.bh_fr_distribute_powers_dev(self.worker.ctx, self._dev, self.m,
                                                    g.ctypes.data_as(ctypes.c_void_p), None))
        self.worker.synchronize()

    def divide_by_z_on_coset(self, worker=None):
        check(self._lib.bh_fr_divide_by_z_on_coset_dev(self.worker.ctx, self._dev, self.exp, None))
        self.worker.synchronize()

    def mul_assign(self, worker, other):
        assert self.m == other.m  # domain.rs:155
        check(self._lib.bh_fr_mul_assign_dev(self.worker.ctx, self._dev, other._dev, self.m, None))
        self.worker.synchronize()

    def sub_assign(self, worker, other):
        assert self.m == other.m  # domain.rs:174
        check(self._lib.bh_fr_sub_assign_dev(self.worker.ctx, self._dev, other._dev, self.m, None))
        self.worker.synchronize()


MANY_FORCE, MANY_SINGLE = C.BH_FFT_MANY_FORCE, C.BH_FFT_MANY_SINGLE


def _pad_all(list_of_coeffs):
    """from_coeffs (domain.rs:47-79) for every member; all must pad to one m"""
    vs = [np.asarray(v, dtype=np.uint64).reshape(-1, 4) for v in list_of_coeffs]
    ms = []
    for v in vs:   # (sizes first: a vector that is too long is refused before anything is copied)
        m, exp = 1, 0
        while m < v.shape[0]:
            m *= 2
            exp += 1
            if exp >= FR_S:
                raise PolynomialDegreeTooLarge()
        ms.append((m, exp))
    if len(set(ms)) > 1:
        raise ValueError("the vectors of an EvaluationDomains must pad to one domain size, got %s" % sorted(set(m for m, _ in ms)))
    m, exp = ms[0] if ms else (1, 0)
    padded = np.zeros((len(vs), m, 4), dtype=np.uint64)
    for j, v in enumerate(vs):
        padded[j, : v.shape[0]] = v
    return padded, m, exp


class EvaluationDomains:
    """k `EvaluationDomain`s of one size, contiguous in HBM: every transform is ONE call over the k vectors
    (bh_fft_fr_many_dev), the element-wise operations run over the k * m elements."""

    def __init__(self, worker, dev, k, m, exp):
        self.worker, self._dev, self.k, self.m, self.exp = worker, dev, k, m, exp
        self._lib = _lib.load()

    @classmethod
    def from_coeffs(cls, worker, list_of_coeffs):
        padded, m, exp = _pad_all(list_of_coeffs)
        k = padded.shape[0]
        dev = worker.alloc(max(k, 1) * m * 32)
        if k:
            worker.upload(dev, padded)
        return cls(worker, dev, k, m, exp)

    def __len__(self):
        return self.k

    def as_ref(self):
        out = np.empty((self.k, self.m, 4), dtype=np.uint64)
        if self.k:
            self.worker.download(out, self._dev)
        return [out[j] for j in range(self.k)]

    def into_coeffs(self):
        out = self.as_ref()
        self.worker.free(self._dev)
        self._dev = None
        return out

    def _fft(self, mode, flags):
        check(self._lib.bh_fft_fr_many_dev(self.worker.ctx, self._dev, self.m * 32, self.k, self.exp, mode, flags, None), "fft")
        self.worker.synchronize()

    def fft(self, worker=None, flags=0):
        self._fft(C.BH_FFT, flags)

    def ifft(self, worker=None, flags=0):
        self._fft(C.BH_IFFT, flags)

    def coset_fft(self, worker=None, flags=0):
        self._fft(C.BH_COSET_FFT, flags)

    def icoset_fft(self, worker=None, flags=0):
        self._fft(C.BH_ICOSET_FFT, flags)

    def divide_by_z_on_coset(self, worker=None):
        """every member by Z(7) (domain.rs:139-151).  The existing call takes a domain size, so it runs once per member."""
        for j in range(self.k):
            member = ctypes.c_void_p(self._dev.value + j * self.m * 32)
            check(self._lib.bh_fr_divide_by_z_on_coset_dev(self.worker.ctx, member, self.exp, None))
        self.worker.synchronize()

    def mul_assign(self, worker, other):
        assert self.m == other.m and self.k == other.k  # domain.rs:155
        check(self._lib.bh_fr_mul_assign_dev(self.worker.ctx, self._dev, other._dev, self.k * self.m, None))
        self.worker.synchronize()

    def sub_assign(self, worker, other):
        assert self.m == other.m and self.k == other.k  # domain.rs:174
        check(self._lib.bh_fr_sub_assign_dev(self.worker.ctx, self._dev, other._dev, self.k * self.m, None))
        self.worker.synchronize()


def h_poly_many(worker, a_list, b_list, c_list, flags=0):
    """The h block of create_proof (groth16/src/prover.rs:221-240) for k proofs of one circuit in one call
    (bh_h_poly_fr_many_dev_on): k arrays of m - 1 quotient coefficients."""
    lib = _lib.load()
    if not (len(a_list) == len(b_list) == len(c_list)):
        raise ValueError("one a, b and c per proof")
    pa, m, exp = _pad_all(a_list)
    pb, mb, _ = _pad_all(b_list)
    pc, mc, _ = _pad_all(c_list)
    if not (m == mb == mc):
        raise ValueError("a, b and c must pad to one domain size")
    k = pa.shape[0]
    if not k:
        return []
    vec = m * 32
    dev = worker.alloc(4 * k * vec)   # a, b, c and a scratch vector per proof
    try:
        at = lambda i: ctypes.c_void_p(dev.value + i * k * vec)  # noqa: E731
        for i, p in enumerate((pa, pb, pc)):
            worker.upload(at(i), p)
        check(lib.bh_h_poly_fr_many_dev_on(worker.ctx, at(0), at(1), at(2), vec, k, exp, flags, at(3), k * vec, None), "h_poly_many")
        worker.synchronize()
        out = np.empty((k, m, 4), dtype=np.uint64)
        worker.download(out, at(0))
    finally:
        worker.free(dev)
    return [out[j, : m - 1].copy() for j in range(k)]


POINT_WORDS = {1: 12, 2: 24}   # u64 words per affine record: G1 96 bytes, G2 192


class PointEvaluationDomain:
    """EvaluationDomain<Fr, Point<G>>: the same methods over group elements (group 1 = G1, 2 = G2).  The ifft of a
    powers-of-tau transcript [tau^i]G gives the Lagrange-basis points [L_j(tau)]G."""

    def __init__(self, worker, group, dev, m, exp):
        self.worker, self.group, self._dev, self.m, self.exp = worker, group, dev, m, exp
        self._lib = _lib.load()

    @classmethod
    def from_coeffs(cls, worker, group, points):
        """domain.rs:47-79: pad to m = next power of two >= len with identity records; exp >= S errors."""
        if group not in POINT_WORDS:
            raise ValueError("group must be 1 (G1) or 2 (G2)")
        words = POINT_WORDS[group]
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
        m, exp = 1, 0
        while m < points.shape[0]:
            m *= 2
            exp += 1
            if exp >= FR_S:
                raise PolynomialDegreeTooLarge()
        if points.shape[0] == m:
            padded = points
        else:
            padded = np.zeros((m, words), dtype=np.uint64)
            padded[: points.shape[0]] = points
        dev = worker.alloc(m * words * 8)
        worker.upload(dev, padded)
        return cls(worker, group, dev, m, exp)

    def __len__(self):
        return self.m

    def as_ref(self):
        out = np.empty((self.m, POINT_WORDS[self.group]), dtype=np.uint64)
        self.worker.download(out, self._dev)
        return out

    def into_coeffs(self):
        out = self.as_ref()
        self.worker.free(self._dev)
        self._dev = None
        return out

    def _fft(self, mode):
        check(self._lib.bh_fft_point_dev(self.worker.ctx, self.group, self._dev, self.exp, mode, None), "point fft")

    def fft(self, worker=None):
        self._fft(C.BH_FFT)

    def ifft(self, worker=None):
        self._fft(C.BH_IFFT)

    def coset_fft(self, worker=None):
        self._fft(C.BH_COSET_FFT)

    def icoset_fft(self, worker=None):
        self._fft(C.BH_ICOSET_FFT)

    def distribute_powers(self, worker, g_mont):
        g = np.ascontiguousarray(g_mont, dtype=np.uint64).reshape(4)
        check(self._lib.bh_point_distribute_powers_dev(self.worker.ctx, self.group, self._dev, self.m,
                                                       g.ctypes.data_as(ctypes.c_void_p), None))

    def divide_by_z_on_coset(self, worker=None):
        check(self._lib.bh_point_divide_by_z_on_coset_dev(self.worker.ctx, self.group, self._dev, self.exp, None))
        self.worker.synchronize()

    def mul_assign(self, worker, other):
        """point_i *= scalar_i with the scalars of an EvaluationDomain (domain.rs:154-170)"""
        assert self.m == other.m  # domain.rs:155
        check(self._lib.bh_point_mul_assign_dev(self.worker.ctx, self.group, self._dev, other._dev, self.m, None))
        self.worker.synchronize()

    def sub_assign(self, worker, other):
        assert self.m == other.m and self.group == other.group  # domain.rs:174
        check(self._lib.bh_point_sub_assign_dev(self.worker.ctx, self.group, self._dev, other._dev, self.m, None))
        self.worker.synchronize()
