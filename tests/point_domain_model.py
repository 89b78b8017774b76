"""Restatement of src/domain.rs for the `Point<G>` instantiation (:192-229): serial_fft, parallel_fft, the four
transforms, distribute_powers and the element-wise operations over GROUP elements, with the group law executed by the C
oracle (oracle.cengine.CGroup).  The group-valued twin of oracle/pyref/domain.py, kept under tests/ because oracle/ is
frozen.  Points are `bytes` records in the library format (96 / 192-byte Montgomery affine, all-zero = identity);
scalars are Python ints mod q."""

import numpy as np

from oracle.cengine import CGroup
from oracle.pyref import bls12_381 as bls
from oracle.pyref.domain import bitreverse
from oracle.pyref.errors import PolynomialDegreeTooLarge

Q = bls.Q
FR_S = bls.FR_S
GENERATOR = bls.FR_GENERATOR


def fp_neg_words(words):
    """-y for a Montgomery Fp element given as 6 little-endian u64 words (the Montgomery form of -y is p - mont(y))"""
    v = 0
    for i, w in enumerate(words):
        v |= int(w) << (64 * i)
    v = (bls.P - v) % bls.P
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


class PointGroup:
    """CGroup plus the negation the domain's sub_assign needs (y -> -y on the record)."""

    def __init__(self, group):
        self.group = group
        self.g = CGroup(group)
        self.words = self.g.words

    def identity(self):
        return self.g.identity()

    def add(self, a, b):
        return self.g.add(a, b)

    def mul(self, a, k):
        k %= Q
        if k == 0 or self.g.is_identity(a):
            return self.g.identity()
        if k == 1:
            return a
        return self.g.mul(a, k)

    def neg(self, a):
        if self.g.is_identity(a):
            return a
        w = np.frombuffer(a, dtype=np.uint64).copy()
        half = self.words // 2   # x | y
        for c in range(half // 6):
            w[half + 6 * c: half + 6 * c + 6] = fp_neg_words(w[half + 6 * c: half + 6 * c + 6])
        return w.tobytes()

    def sub(self, a, b):
        return self.add(a, self.neg(b))

    def gen(self):
        return self.g.gen

    def records(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, self.words)
        return [row.tobytes() for row in arr]

    def to_array(self, pts):
        return self.g.to_array(list(pts))


def serial_fft(G, a, omega, log_n):
    """domain.rs:272-314 over group elements (in place on list `a`)."""
    n = len(a)
    assert n == 1 << log_n
    for k in range(n):
        rk = bitreverse(k, log_n)
        if k < rk:
            a[rk], a[k] = a[k], a[rk]
    m = 1
    for _ in range(log_n):
        w_m = pow(omega, n // (2 * m), Q)
        k = 0
        while k < n:
            w = 1
            for j in range(m):
                t = G.mul(a[k + j + m], w)
                a[k + j + m] = G.sub(a[k + j], t)
                a[k + j] = G.add(a[k + j], t)
                w = (w * w_m) % Q
            k += 2 * m
        m *= 2


def parallel_fft(G, a, omega, log_n, log_cpus):
    """domain.rs:316-372 over group elements (executed serially; the split is what matters)."""
    assert log_n >= log_cpus
    num_cpus = 1 << log_cpus
    log_new_n = log_n - log_cpus
    tmp = [[G.identity()] * (1 << log_new_n) for _ in range(num_cpus)]
    new_omega = pow(omega, num_cpus, Q)
    for j in range(num_cpus):
        omega_j = pow(omega, j, Q)
        omega_step = pow(omega, j << log_new_n, Q)
        elt = 1
        t_j = tmp[j]
        for i in range(1 << log_new_n):
            for s in range(num_cpus):
                idx = (i + (s << log_new_n)) % (1 << log_n)
                t_j[i] = G.add(t_j[i], G.mul(a[idx], elt))
                elt = (elt * omega_step) % Q
            elt = (elt * omega_j) % Q
        serial_fft(G, t_j, new_omega, log_new_n)
    mask = (1 << log_cpus) - 1
    for idx in range(len(a)):
        a[idx] = tmp[idx & mask][idx >> log_cpus]


def best_fft(G, a, omega, log_n, log_cpus=0):
    """domain.rs:261-269"""
    if log_n <= log_cpus:
        serial_fft(G, a, omega, log_n)
    else:
        parallel_fft(G, a, omega, log_n, log_cpus)


def dft(G, points, omega):
    """the definition: out_j = sum_i [omega^(i j)] P_i"""
    n = len(points)
    out = []
    for j in range(n):
        acc = G.identity()
        for i, p in enumerate(points):
            acc = G.add(acc, G.mul(p, pow(omega, i * j, Q)))
        out.append(acc)
    return out


class PointDomain:
    """EvaluationDomain<Fr, Point<G>> (domain.rs:21-229)."""

    def __init__(self, G, coeffs, exp, log_cpus=0):
        self.G, self.coeffs, self.exp, self.log_cpus = G, coeffs, exp, log_cpus
        omega = bls.FR_ROOT_OF_UNITY
        for _ in range(exp, FR_S):
            omega = omega * omega % Q
        self.omega = omega
        self.omegainv = pow(omega, -1, Q)
        self.geninv = pow(GENERATOR, -1, Q)
        self.minv = pow(len(coeffs) % Q, -1, Q)

    @classmethod
    def from_coeffs(cls, G, coeffs, log_cpus=0):
        """domain.rs:47-79: pad with the identity"""
        n = len(coeffs)
        m, exp = 1, 0
        while m < n:
            m *= 2
            exp += 1
            if exp >= FR_S:
                raise PolynomialDegreeTooLarge()
        coeffs = list(coeffs)
        coeffs.extend([G.identity()] * (m - len(coeffs)))
        return cls(G, coeffs, exp, log_cpus)

    def __len__(self):
        return len(self.coeffs)

    def fft(self):
        best_fft(self.G, self.coeffs, self.omega, self.exp, self.log_cpus)

    def ifft(self):
        best_fft(self.G, self.coeffs, self.omegainv, self.exp, self.log_cpus)
        self.coeffs = [self.G.mul(p, self.minv) for p in self.coeffs]

    def distribute_powers(self, g):
        """domain.rs:101-113 (the chunking of Worker::scope does not change the result)"""
        u = 1
        for k in range(len(self.coeffs)):
            self.coeffs[k] = self.G.mul(self.coeffs[k], u)
            u = u * g % Q

    def coset_fft(self):
        self.distribute_powers(GENERATOR)
        self.fft()

    def icoset_fft(self):
        self.ifft()
        self.distribute_powers(self.geninv)

    def z(self, tau):
        return (pow(tau, len(self.coeffs), Q) - 1) % Q

    def divide_by_z_on_coset(self):
        i = pow(self.z(GENERATOR), -1, Q)
        self.coeffs = [self.G.mul(p, i) for p in self.coeffs]

    def mul_assign(self, scalars):
        """domain.rs:154-170 with other = an EvaluationDomain<Scalar> (ints)"""
        assert len(scalars) == len(self.coeffs)
        self.coeffs = [self.G.mul(p, s) for p, s in zip(self.coeffs, scalars)]

    def sub_assign(self, other):
        """domain.rs:173-189"""
        assert len(other) == len(self.coeffs)
        self.coeffs = [self.G.sub(a, b) for a, b in zip(self.coeffs, other)]

    def run(self, mode):
        (self.fft, self.ifft, self.coset_fft, self.icoset_fft)[mode]()
