"""k proofs of one circuit in one call (bh_groth16_prove_witness_batch, groth16.prove_witness_batch) on the GPU: every
proof is the single call's and the oracle's, byte for byte; a witness of the wrong shape is refused before anything runs;
the group cut under a small workspace budget changes nothing.  Both ways of running the call are checked: the product's
(proofs in flight) and the grouped path behind it (five many-jobs per group of witnesses; _workspace_budget=0 takes it
with the default budget)."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cprover, cref  # noqa: E402
from oracle.cengine import CBls12  # noqa: E402
from oracle.pyref.generator import generate_parameters  # noqa: E402
from tests import circuits  # noqa: E402

TOXIC = dict(alpha=48577, beta=22580, gamma=53332, delta=5481, tau=3673)


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


def _product_params(worker, p):
    from bellman_amd import groth16 as pg

    G1, G2 = CBls12.G1, CBls12.G2
    arr = lambda b: np.frombuffer(b, dtype=np.uint64)  # noqa: E731
    return pg.Parameters(worker, arr(p.vk.alpha_g1), arr(p.vk.beta_g1), arr(p.vk.beta_g2), arr(p.vk.delta_g1), arr(p.vk.delta_g2),
                         G1.to_array(p.h), G1.to_array(p.l), G1.to_array(p.a), G1.to_array(p.b_g1), G2.to_array(p.b_g2))


def _same(proof, a, b, c):
    return proof.a.tobytes() == bytes(a) and proof.b.tobytes() == bytes(b) and proof.c.tobytes() == bytes(c)


def _chain_setup(worker, rounds, seed):
    """synthetic CRS for the chain circuit (distinct prime-order points; parity only)"""
    from bellman_amd import groth16 as pg

    n_cons = rounds + 3
    m = 1
    while m < n_cons:
        m *= 2
    n_aux = rounds + 1
    nb = (rounds + 1) // 2 + 2
    h, l, a = cref.gen_bases(1, m - 1, a=11, b=3), cref.gen_bases(1, n_aux, a=5, b=7), cref.gen_bases(1, n_aux + 2, a=2, b=9)
    b1, b2 = cref.gen_bases(1, nb, a=13, b=4), cref.gen_bases(2, nb, a=17, b=6)
    g1, g2 = cref.g1_generator(), cref.g2_generator()
    vk = dict(alpha_g1=cref.point_mul(1, g1, 101), beta_g1=cref.point_mul(1, g1, 102), beta_g2=cref.point_mul(2, g2, 102),
              delta_g1=cref.point_mul(1, g1, 103), delta_g2=cref.point_mul(2, g2, 103))
    pp = pg.Parameters(worker, vk["alpha_g1"], vk["beta_g1"], vk["beta_g2"], vk["delta_g1"], vk["delta_g2"], h, l, a, b1, b2)
    return pp, vk, (h, l, a, b1, b2)


Q = circuits.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "prove_batch_cubic.bin")


def _witness(circuit):
    from bellman_amd import groth16 as pg

    w = pg.WitnessAssignment()
    w.alloc_input(lambda: 1)
    circuit(w)
    return w.input_assignment, w.aux_assignment


def _equal(p, q):
    return np.array_equal(p.a, q.a) and np.array_equal(p.b, q.b) and np.array_equal(p.c, q.c)


def _oracle_proof(p, circuit, r, s):
    """the oracle's create_proof for a Python circuit: its synthesis restated in integers (prover.rs:182-215), then the C
    restatement of prover.rs:217-360 (oracle/cprover.py, pinned against oracle/pyref by tests/test_oracle_c_vs_pyref.py) -
    the pure-Python prover takes five seconds per MiMC proof"""
    from bellman_amd import groth16 as pg

    G1, G2 = CBls12.G1, CBls12.G2
    pa = pg.ProvingAssignment()
    pa.alloc_input(lambda: 1)
    circuit(pa)
    for i in range(len(pa.input_assignment)):
        pa.enforce(lambda lc, i=i: lc + pg.Variable(pg.INPUT, i), lambda lc: lc, lambda lc: lc)
    arr = lambda b: np.frombuffer(b, dtype=np.uint64)  # noqa: E731
    vk = dict(alpha_g1=arr(p.vk.alpha_g1), beta_g1=arr(p.vk.beta_g1), beta_g2=arr(p.vk.beta_g2), delta_g1=arr(p.vk.delta_g1),
              delta_g2=arr(p.vk.delta_g2))
    return cprover.prove_assignment(pa.a, pa.b, pa.c, pa.input_assignment, pa.aux_assignment, pa.a_aux_density.bv,
                                    pa.b_input_density.bv, pa.b_aux_density.bv, vk, G1.to_array(p.h), G1.to_array(p.l),
                                    G1.to_array(p.a), G1.to_array(p.b_g1), G2.to_array(p.b_g2), r, s)


@pytest.mark.gpu
def test_mimc_322_batch(worker):
    """k = 5 witnesses with different (xl, xr, r, s): every proof equals the oracle's; k = 1 equals prove_witness"""
    from bellman_amd import groth16 as pg

    rnd = random.Random(322)
    cons = [rnd.randrange(Q) for _ in range(circuits.MIMC_ROUNDS)]
    p = generate_parameters(CBls12, circuits.mimc_circuit(0, 0, cons), CBls12.G1.gen, CBls12.G2.gen, **TOXIC)
    pp = _product_params(worker, p)
    r1cs = pg.R1CS.from_circuit(worker, circuits.mimc_circuit(0, 0, cons))
    k = 5
    cases = [tuple(rnd.randrange(Q) for _ in range(4)) for _ in range(k)]   # xl, xr, r, s
    wits = [_witness(circuits.mimc_circuit(xl, xr, cons)) for xl, xr, _, _ in cases]
    got = pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], [c[2] for c in cases], [c[3] for c in cases])
    grouped = pg.prove_witness_batch(r1cs, pp, [w[0] for w in wits], [w[1] for w in wits], [c[2] for c in cases],
                                     [c[3] for c in cases], _workspace_budget=0)
    assert len(got) == k and len(grouped) == k
    for (xl, xr, r, s), g, g2 in zip(cases, got, grouped):
        want = _oracle_proof(p, circuits.mimc_circuit(xl, xr, cons), r, s)
        assert _same(g, want[0].tobytes(), want[1].tobytes(), want[2].tobytes())
        assert _same(g2, want[0].tobytes(), want[1].tobytes(), want[2].tobytes())
    one = pg.prove_witness_batch(r1cs, pp, [wits[2][0]], [wits[2][1]], [cases[2][2]], [cases[2][3]])
    assert len(one) == 1 and _equal(one[0], pg.prove_witness(r1cs, pp, wits[2][0], wits[2][1], cases[2][2], cases[2][3]))
    assert _equal(one[0], got[2])
    assert pg.prove_witness_batch(r1cs, pp, [], [], [], []) == []
    r1cs.release()


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [1, 61, 4093])
def test_chain_batch(worker, rounds):
    from bellman_amd import groth16 as pg

    seed, k = 7 + rounds, 3
    pp, vk, (h, l, a, b1, b2) = _chain_setup(worker, rounds, seed)
    r1cs = pg.R1CS.from_demo(worker, 1, rounds, seed)
    fs = [circuits.chain_assignment_fast(rounds, seed, 123456789 + 1000 * j) for j in range(k)]
    rs = [0x1234567 + rounds + j for j in range(k)]
    ss = [0x7654321 + 3 * j for j in range(k)]
    got = pg.prove_witness_batch(r1cs, pp, [f["input_assignment"] for f in fs], [f["aux_assignment"] for f in fs], rs, ss)
    grouped = pg.prove_witness_batch(r1cs, pp, [f["input_assignment"] for f in fs], [f["aux_assignment"] for f in fs], rs, ss,
                                     _workspace_budget=0)
    for j, f in enumerate(fs):
        want = cprover.prove_assignment(f["a"], f["b"], f["c"], f["input_assignment"], f["aux_assignment"], f["a_aux_density"],
                                        f["b_input_density"], f["b_aux_density"], vk, h, l, a, b1, b2, rs[j], ss[j])
        assert _same(got[j], want[0].tobytes(), want[1].tobytes(), want[2].tobytes()), j
        assert _same(grouped[j], want[0].tobytes(), want[1].tobytes(), want[2].tobytes()), j
    r1cs.release()


@pytest.fixture(scope="module")
def boolmix(worker):
    """the boolean circuit at its smallest size, with generated (valid) parameters, four witnesses and the single call's proofs"""
    from bellman_amd import groth16 as pg
    from bellman_amd import verifier

    rounds, seed = circuits.boolmix_rounds(7), 31
    rnd = random.Random(5)
    r1cs = pg.R1CS.from_demo(worker, 5, rounds, seed)
    g1, g2 = cref.g1_generator(), cref.g2_generator()
    params = pg.Parameters.generate(worker, r1cs, g1, g2, *[rnd.randrange(1, Q) for _ in range(5)])
    fs = [circuits.boolmix_assignment_fast(rounds, seed, 0x0123456789ABCDEF + 77 * j) for j in range(7)]
    rs = [rnd.randrange(Q) for _ in fs]
    ss = [rnd.randrange(Q) for _ in fs]
    singles = [pg.prove_witness(r1cs, params, f["input_assignment"], f["aux_assignment"], r, s) for f, r, s in zip(fs, rs, ss)]
    pvk = verifier.prepare_verifying_key(params)
    yield dict(r1cs=r1cs, params=params, fs=fs, rs=rs, ss=ss, singles=singles, pvk=pvk)
    pvk.release()
    r1cs.release()


@pytest.mark.gpu
def test_boolean_circuit_batch_verifies(boolmix):
    from bellman_amd import groth16 as pg
    from bellman_amd import verify_proof

    b, k = boolmix, 4
    got = pg.prove_witness_batch(b["r1cs"], b["params"], [f["input_assignment"] for f in b["fs"][:k]],
                                 [f["aux_assignment"] for f in b["fs"][:k]], b["rs"][:k], b["ss"][:k])
    grouped = pg.prove_witness_batch(b["r1cs"], b["params"], [f["input_assignment"] for f in b["fs"][:k]],
                                     [f["aux_assignment"] for f in b["fs"][:k]], b["rs"][:k], b["ss"][:k], _workspace_budget=0)
    for j in range(k):
        assert _equal(got[j], b["singles"][j]) and _equal(grouped[j], b["singles"][j]), j
        verify_proof(b["pvk"], got[j], b["fs"][j]["input_assignment"][1:])


@pytest.mark.gpu
def test_wrong_shape_refuses_the_whole_call(boolmix):
    """a witness of the wrong shape in slot 2 of 4: InvalidArg for the call, as the single call refuses it"""
    from bellman_amd import groth16 as pg

    b = boolmix
    ins = [f["input_assignment"] for f in b["fs"][:4]]
    auxs = [list(f["aux_assignment"]) for f in b["fs"][:4]]
    auxs[2] = auxs[2][:-1]
    with pytest.raises(AssertionError):
        pg.prove_witness(b["r1cs"], b["params"], ins[2], auxs[2], b["rs"][2], b["ss"][2])
    with pytest.raises(AssertionError):
        pg.prove_witness_batch(b["r1cs"], b["params"], ins, auxs, b["rs"][:4], b["ss"][:4])
    ins[2] = ins[2] + [5]
    with pytest.raises(AssertionError):
        pg.prove_witness_batch(b["r1cs"], b["params"], ins, [f["aux_assignment"] for f in b["fs"][:4]], b["rs"][:4], b["ss"][:4])


@pytest.mark.gpu
def test_group_cut_under_a_small_budget(boolmix):
    """k = 7 over a workspace budget that fits 3 witnesses (groups of 3, 3, 1): the proofs do not change"""
    from bellman_amd import groth16 as pg

    b, k = boolmix, 7
    m = 1
    while m < b["r1cs"].num_constraints:
        m *= 2
    budget = (3 + 3) * m * 32   # three coefficient vectors + the shared b, c and scratch vectors
    got = pg.prove_witness_batch(b["r1cs"], b["params"], [f["input_assignment"] for f in b["fs"]],
                                 [f["aux_assignment"] for f in b["fs"]], b["rs"], b["ss"], _workspace_budget=budget)
    tiny = pg.prove_witness_batch(b["r1cs"], b["params"], [f["input_assignment"] for f in b["fs"]],
                                  [f["aux_assignment"] for f in b["fs"]], b["rs"], b["ss"], _workspace_budget=1)
    for j in range(k):
        assert _equal(got[j], b["singles"][j]) and _equal(tiny[j], b["singles"][j]), j


def _build_cpp():
    from bellman_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = os.path.join(ROOT, "bellman_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "prove_batch_cubic.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", BIN, os.path.join(lib, "libbellman_groth16.a"), "-L" + lib,
                           "-lbellman_hip", "-Wl,-rpath," + lib, "-lpthread"])


def test_cpp_prove_witness_batch_example_builds():
    _build_cpp()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_prove_witness_batch_matches_prove_witness(tmp_path):
    """groth16::prove_witness_batch in the C++ mirror against groth16::prove_witness (tests/cpp/prove_batch_cubic.cpp)"""
    _build_cpp()
    f = tmp_path / "gens.bin"
    f.write_bytes(cref.g1_generator().tobytes() + cref.g2_generator().tobytes())
    r = subprocess.run([BIN, str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == "prove_witness_batch ok"
