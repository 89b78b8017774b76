"""EvaluationDomain<Fr, Point<G>> without a GPU: the group-valued model of tests/point_domain_model.py against the DFT
definition (pure-Python affine arithmetic of oracle/pyref/bls12_381.py) and against the scalar transform lifted to the
group, plus the C ABI declarations of the device entry points."""

import os
import random
import re

import pytest

from oracle import cref
from oracle.pyref import bls12_381 as bls
from oracle.pyref import domain as sdomain
from oracle.pyref.engines import ScalarField
from oracle.pyref.errors import PolynomialDegreeTooLarge
from tests import point_domain_model as pdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = bls.Q
FIELD = ScalarField(bls.Q, bls.FR_NUM_BITS, bls.FR_S, bls.FR_GENERATOR, bls.FR_ROOT_OF_UNITY)


def _py(G, rec):
    """library record -> pyref affine point (None = identity)"""
    arr = G.to_array([rec])
    return (cref.g1_to_py if G.group == 1 else cref.g2_to_py)(arr)[0]


def _points(G, coeffs):
    return [G.mul(G.gen(), c) for c in coeffs]


def _omega(log_n):
    w = bls.FR_ROOT_OF_UNITY
    for _ in range(log_n, bls.FR_S):
        w = w * w % Q
    return w


class _Worker:
    def __init__(self, log_cpus):
        self.log_cpus = log_cpus

    def log_num_threads(self):
        return self.log_cpus

    def chunk_size(self, n):
        return max(1, n >> self.log_cpus)


@pytest.mark.parametrize("group,log_n", [(1, k) for k in range(5)] + [(2, k) for k in range(4)])
def test_model_fft_is_the_dft(group, log_n):
    """out_j = sum_i [omega^(i j)] P_i, evaluated with the pure-Python affine group law"""
    G = pdm.PointGroup(group)
    curve = bls.G1 if group == 1 else bls.G2
    rnd = random.Random(100 + 10 * group + log_n)
    n = 1 << log_n
    coeffs = [rnd.randrange(Q) for _ in range(n)]
    pts = _points(G, coeffs)
    d = pdm.PointDomain.from_coeffs(G, pts)
    d.fft()
    omega = _omega(log_n)
    py_pts = [_py(G, p) for p in pts]
    for j in range(n):
        acc = None
        for i, p in enumerate(py_pts):
            acc = curve.add(acc, curve.mul(p, pow(omega, i * j, Q)))
        assert _py(G, d.coeffs[j]) == acc, j


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("log_n", range(5))
@pytest.mark.parametrize("mode", range(4))
def test_model_is_the_scalar_transform_lifted(group, log_n, mode):
    """P_i = [c_i]G: every transform of the points is [transform(c)_j]G (oracle/pyref/domain.py for the scalars)"""
    G = pdm.PointGroup(group)
    rnd = random.Random(7 * log_n + mode + 50 * group)
    n = 1 << log_n
    coeffs = [rnd.randrange(Q) for _ in range(n)]
    coeffs[rnd.randrange(n)] = 0   # an identity among the inputs
    d = pdm.PointDomain.from_coeffs(G, _points(G, coeffs))
    d.run(mode)
    s = sdomain.EvaluationDomain.from_coeffs(FIELD, coeffs)
    (s.fft, s.ifft, s.coset_fft, s.icoset_fft)[mode](_Worker(0))
    assert d.coeffs == _points(G, s.coeffs)


@pytest.mark.parametrize("log_cpus", [1, 2])
def test_model_parallel_fft_equals_serial(log_cpus):
    G = pdm.PointGroup(1)
    rnd = random.Random(log_cpus)
    pts = _points(G, [rnd.randrange(Q) for _ in range(16)])
    a, b = list(pts), list(pts)
    pdm.serial_fft(G, a, _omega(4), 4)
    pdm.parallel_fft(G, b, _omega(4), 4, log_cpus)
    assert a == b


def test_model_elementwise_ops():
    G = pdm.PointGroup(1)
    rnd = random.Random(3)
    c = [rnd.randrange(Q) for _ in range(8)]
    e = [rnd.randrange(Q) for _ in range(8)]
    k = [rnd.randrange(Q) for _ in range(8)]
    g = rnd.randrange(1, Q)
    d = pdm.PointDomain.from_coeffs(G, _points(G, c))
    d.distribute_powers(g)
    assert d.coeffs == _points(G, [ci * pow(g, i, Q) for i, ci in enumerate(c)])
    d.mul_assign(k)
    assert d.coeffs == _points(G, [ci * pow(g, i, Q) * ki for i, (ci, ki) in enumerate(zip(c, k))])
    d.sub_assign(_points(G, e))
    assert d.coeffs == _points(G, [ci * pow(g, i, Q) * ki - ei for i, (ci, ki, ei) in enumerate(zip(c, k, e))])
    d.divide_by_z_on_coset()
    zinv = pow(pow(bls.FR_GENERATOR, 8, Q) - 1, -1, Q)
    assert d.coeffs == _points(G, [(ci * pow(g, i, Q) * ki - ei) * zinv for i, (ci, ki, ei) in enumerate(zip(c, k, e))])
    # a - a, a - (-a), identity operands
    p = G.mul(G.gen(), 5)
    assert G.sub(p, p) == G.identity()
    assert G.sub(p, G.neg(p)) == G.mul(G.gen(), 10)
    assert G.sub(G.identity(), p) == G.neg(p)


def test_model_padding_and_degree_limit():
    G = pdm.PointGroup(2)
    pts = _points(G, [3, 4, 5])
    d = pdm.PointDomain.from_coeffs(G, pts)
    assert len(d) == 4 and d.exp == 2 and d.coeffs[3] == G.identity()
    with pytest.raises(PolynomialDegreeTooLarge):
        pdm.PointDomain.from_coeffs(G, _Huge())


class _Huge(list):
    """a list that claims 2^32 + 1 entries without holding them (from_coeffs measures it before copying)"""

    def __len__(self):
        return (1 << 32) + 1


def test_header_declares_the_point_domain_entry_points():
    with open(os.path.join(ROOT, "include", "bellman_hip.h")) as f:
        hdr = f.read()
    want = {
        "bh_fft_point_dev": "bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, int mode, void *stream",
        "bh_point_distribute_powers_dev": "bh_ctx *ctx, int group, void *points_dev, size_t n, const void *g_host, void *stream",
        "bh_point_divide_by_z_on_coset_dev": "bh_ctx *ctx, int group, void *points_dev, uint32_t log_n, void *stream",
        "bh_point_mul_assign_dev": "bh_ctx *ctx, int group, void *points_dev, const void *scalars_dev, size_t n, void *stream",
        "bh_point_sub_assign_dev": "bh_ctx *ctx, int group, void *a_dev, const void *b_dev, size_t n, void *stream",
    }
    for name, args in want.items():
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        assert " ".join(m.group(1).split()) == args, name
