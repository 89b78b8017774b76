"""Witnesses of gadget circuits computed on the GPU from their word program (bh_word_witness_create /
bh_word_witness_generate_dev / bh_word_witness_generate; bellman_amd.gadgets.WordWitness): every byte of every witness equals
host synthesis of the same circuit with the same external words - for one circuit per instruction kind (tests/models/
word_circuits.py) with k on the edges of a wavefront, padded strides that must come back untouched and a forced scratch chunk
that k crosses, and for Sha256Preimage at one and two blocks and doubled, where the result also equals what the witness solver
makes of the same circuit, satisfies every constraint and exposes hashlib's digest.  The generated buffers then go unchanged
into prove_witness_batch_dev(check=True)."""
import hashlib
import random

import numpy as np
import pytest

from tests.models import word_circuits as wc

pytestmark = pytest.mark.gpu

KS = (1, 63, 64, 65, 130)
SENTINEL = 0x5A5A5A5A5A5A5A5A   # DeviceWitnesses.from_host's padding pattern
K_SHA = 3


@pytest.fixture(scope="module")
def worker():
    import bellman_amd

    w = bellman_amd.Worker(0)
    yield w
    w.close()


_ONE_OP = {}


def _one_op(worker, kind):
    """per module and kind: (shape, generator, ext rows [130, n_ext], host witnesses of all 130 rows)"""
    from bellman_amd import gadgets as g

    if kind not in _ONE_OP:
        c = wc.OneOp(kind)
        shape = g.capture(c)
        rows = wc.ext_rows(kind, max(KS))
        _ONE_OP[kind] = (shape, shape.witness_generator(worker), rows, wc.host_witnesses(c.with_ext, rows))
    return _ONE_OP[kind]


def _check_images(w, want_in, want_aux, k, stride_extra):
    raw_in, raw_aux = w.download_raw()
    n_in, n_aux = want_in.shape[1], want_aux.shape[1]
    assert raw_in.shape == (k, n_in * 4 + stride_extra // 8) and raw_aux.shape == (k, n_aux * 4 + stride_extra // 8)
    assert np.array_equal(raw_in[:, :n_in * 4], want_in[:k].reshape(k, -1)), "inputs"
    assert np.array_equal(raw_aux[:, :n_aux * 4], want_aux[:k].reshape(k, -1)), "aux"
    assert (raw_in[:, n_in * 4:] == SENTINEL).all() and (raw_aux[:, n_aux * 4:] == SENTINEL).all(), "stride padding written"


@pytest.mark.parametrize("kind", wc.KINDS)
def test_one_op_circuits_equal_host_synthesis(worker, kind):
    shape, gen, rows, (want_in, want_aux) = _one_op(worker, kind)
    assert 64 <= shape.num_aux <= 1200
    for k in KS:
        for stride_extra, chunk in ((0, 0), (96, 0)) + (((32, 48),) if k == 130 else ()):
            w = gen.generate_dev(rows[:k], stride_extra=stride_extra, _chunk=chunk)   # 48: k = 130 crosses two chunk ends
            try:
                _check_images(w, want_in, want_aux, k, stride_extra)
            finally:
                w.release()
    gen.generate_dev(rows[:1], _chunk=0).release()
    if kind == "packed_input":   # the all-ones 254-bit pack, 2^254 - 1 < q, and the 2-bit one
        from bellman_amd.groth16 import fr_to_mont_array

        assert want_in[1].tobytes() == fr_to_mont_array([1, (1 << 254) - 1, 3]).tobytes()


def test_host_form_equals_device_form(worker):
    for kind in ("add10", "packed_input"):
        shape, gen, rows, (want_in, want_aux) = _one_op(worker, kind)
        ins, aux = gen.generate(rows[:65])
        assert np.array_equal(ins, want_in[:65]) and np.array_equal(aux, want_aux[:65])
        w = gen.generate_dev(rows[:65])
        try:
            d_in, d_aux = w.download()
        finally:
            w.release()
        assert np.array_equal(ins, d_in) and np.array_equal(aux, d_aux)
        assert gen.generate(rows[:0])[1].shape == (0, shape.num_aux, 4)
    with pytest.raises(ValueError):
        gen.generate(rows[:, :3])


def test_create_refuses_a_bad_program_with_its_index(worker):
    from bellman_amd import gadgets as g

    shape = _one_op(worker, "xor")[0]
    p = dict(shape.program)
    p["bit_vars"] = p["bit_vars"][:-1]   # the last variable loses its record
    with pytest.raises(g.WordProgramError) as e:
        g.WordWitness(worker, shape.num_inputs, shape.num_aux, p)
    assert (e.value.code, e.value.index) == (g.BAD_UNCOVERED, int(shape.program["bit_vars"][-1][0]))


_SHA = {}


def _sha(worker, n, double=False):
    from bellman_amd import gadgets as g

    key = (n, double)
    if key not in _SHA:
        c = g.Sha256Preimage(n, double)
        rnd = random.Random(100 * n + double)
        msgs = [bytes(n), b"\xff" * n, bytes(rnd.getrandbits(8) for _ in range(n))]
        shape = g.capture(c)
        want = wc.host_witnesses(lambda m: c.with_message(m), msgs)
        _SHA[key] = (c, shape, shape.r1cs(worker), shape.witness_generator(worker), msgs, want)
    return _SHA[key]


@pytest.mark.parametrize("n,double,blocks", [(1, False, 1), (55, False, 1), (56, False, 2), (64, False, 2), (32, True, 2)])
def test_sha256_preimage(worker, n, double, blocks):
    from bellman_amd import gadgets as g
    from bellman_amd.groth16 import DeviceWitnesses, fr_to_mont_array

    c, shape, r1cs, gen, msgs, (want_in, want_aux) = _sha(worker, n, double)
    assert (n + 9 + 63) // 64 + (1 if double else 0) == blocks and not shape.untagged
    assert (r1cs.num_inputs, r1cs.num_aux) == (3, shape.num_aux)
    w = gen.generate_dev(c.ext_from_messages(msgs), stride_extra=64)
    try:
        _check_images(w, want_in, want_aux, K_SHA, 64)                      # 1: equals host synthesis, byte for byte
        got_in, got_aux = w.download()
    finally:
        w.release()
    # 2: equals what the solver makes of ONE and the message bits on the same circuit
    solver = shape.solver(r1cs)
    start_in, start_aux = np.zeros_like(want_in), np.zeros_like(want_aux)
    start_in[:, 0] = want_in[:, 0]
    sup = [v.idx for v in shape.supplied]
    assert len(sup) == 8 * n and all(v.kind == 1 for v in shape.supplied)
    start_aux[:, sup] = want_aux[:, sup]
    ws = DeviceWitnesses.from_host(worker, start_in, start_aux)
    try:
        solver.solve_many_dev(ws)
        s_in, s_aux = ws.download()
    finally:
        ws.release()
        solver.release()
    assert np.array_equal(s_in, got_in) and np.array_equal(s_aux, got_aux)
    assert r1cs.which_is_unsatisfied(got_in, got_aux) == [None] * K_SHA       # 3
    for j, m in enumerate(msgs):                                              # 4: the inputs are hashlib's digest, packed
        d = hashlib.sha256(m).digest()
        d = hashlib.sha256(d).digest() if double else d
        packed = g.compute_multipacking(g.bytes_to_bits(d))
        assert packed == c.public_inputs(m) and got_in[j].tobytes() == fr_to_mont_array([1] + packed).tobytes()


def test_generated_witnesses_prove_and_verify(worker):
    from bellman_amd import gadgets as g, verifier
    from bellman_amd import groth16 as pg
    from bellman_amd.errors import Unsatisfiable
    from oracle import cref

    c, shape, r1cs, gen, msgs, (want_in, want_aux) = _sha(worker, 55)
    rnd = random.Random(55)
    params = pg.Parameters.generate(worker, r1cs, cref.g1_generator(), cref.g2_generator(), *[rnd.randrange(1, pg.Q) for _ in range(5)])
    rs, ss = [rnd.randrange(pg.Q) for _ in msgs], [rnd.randrange(pg.Q) for _ in msgs]
    w = gen.generate_dev(c.ext_from_messages(msgs))
    try:
        proofs = pg.prove_witness_batch_dev(r1cs, params, w, rs, ss, check=True)
    finally:
        w.release()
    for j in range(K_SHA):
        host_in, host_aux = g.synthesize(c.with_message(msgs[j]))
        assert proofs[j].write() == pg.prove_witness(r1cs, params, host_in, host_aux, rs[j], ss[j]).write()
    pvk = verifier.prepare_verifying_key(params)
    assert verifier.verify_each(pvk, [(p, c.public_inputs(m)) for p, m in zip(proofs, msgs)]) == [None] * K_SHA
    wrong = verifier.verify_each(pvk, [(proofs[0], c.public_inputs(msgs[1]))])
    assert wrong[0] is not None and wrong[0].__class__.__name__ == "InvalidProof"
    # a message bit flipped after generation (the host form, then the edit): that witness alone is refused
    ins, aux = gen.generate(c.ext_from_messages(msgs))
    one, zero = pg.fr_to_mont_array([1, 0])
    flipped = shape.supplied[100].idx
    aux[1, flipped] = zero if aux[1, flipped].tobytes() == one.tobytes() else one
    bad = pg.DeviceWitnesses.from_host(worker, ins, aux)
    try:
        codes, first = [], []
        got = pg.prove_witness_batch_dev(r1cs, params, bad, rs, ss, check=True, _codes=codes, _first_unsatisfied=first)
        assert codes == [0, 11, 0] and got[1] is None and first[0] is None and first[2] is None and first[1] is not None
        assert got[0].write() == proofs[0].write() and got[2].write() == proofs[2].write()
        with pytest.raises(Unsatisfiable) as e:
            pg.prove_witness_batch_dev(r1cs, params, bad, rs, ss, check=True)
        assert e.value.index == first[1]
    finally:
        bad.release()
        pvk.release()
        params.release()
