"""Proofs of several verifying keys in one call (bh_groth16_*_keys): the exponent model of the batch check over
tests/models/pairing_stage_model.ScalarKey, and the host's grouping of a chunk's rows by key (csrc/pairing.hip Grouping) on
Python lists.  tests/test_keyset_cpu.py pins the exponent model; tests/test_gpu_verify_keys.py and
tests/test_gpu_verify_keys_stages.py use both.

With a ScalarKey's discrete logs (alpha = [a] G1, beta = [b] G2, gamma = [g] G2, delta = [d] G2, ic_i = [c_i] G1) and a
proof A = [r] G1, B = [s] G2, C = [c] G1, the value whose being 1 is the proof's verification equation is e(G1, G2)^E with
    E = r s - a b - (c_0 + sum x_i c_i) g - c d   (mod q),
and the batch check over rows j with the caller's z_j passes exactly when sum_j z_j E_j = 0 (mod q), whatever the keys."""

import random

from tests import group_model as gm
from tests.models import pairing_stage_model as psm

Q = psm.Q


def proof_with_logs(key, inputs):
    """key.proof(inputs) and the discrete logs (r, s, c) of its points: the draws of r and s are replayed from the state of
    the key's generator, c follows from E = 0"""
    replay = random.Random()
    replay.setstate(key.rnd.getstate())
    proof = key.proof(inputs)
    r, s = replay.randrange(1, Q), replay.randrange(1, Q)
    acc = (key.c[0] + sum(x * k for x, k in zip(inputs, key.c[1:]))) % Q
    c = (r * s - key.a * key.b - acc * key.g) * pow(key.d, -1, Q) % Q
    return proof, (r, s, c)


def exponent(key, logs, inputs):
    r, s, c = logs
    acc = key.c[0] + sum(x * k for x, k in zip(inputs, key.c[1:]))
    return (r * s - key.a * key.b - acc * key.g - c * key.d) % Q


def shift_c(proof, t):
    """C += [t] G1"""
    return proof[0], proof[1], gm.add(1, proof[2], gm.mul(1, gm.GEN[1], t % Q))


def batch_exponent(terms):
    """terms: (z_j, E_j) -> the exponent of the batch's product"""
    return sum(z * e for z, e in terms) % Q


def cancelling_shift(key1, z1, t1, key2, z2):
    """t2 with z1 (-t1 d1) + z2 (-t2 d2) = 0: a bad proof under key2 that hides the bad proof under key1 from whoever
    fixed z beforehand"""
    return (-z1 * t1 * key1.d) * pow(z2 * key2.d, -1, Q) % Q


# ---------------------------------------------------------------------------------------------- grouping a chunk by key
def group_rows(key_of, n_inputs):
    """key_of[j] for the rows of one chunk, n_inputs[k] per key -> (perm, segs, blocks): grouped row r is the caller's row
    perm[r] (a stable counting sort); segs[k] = (first row, row count, first scalar); blocks = (key, first row, rows <= 64,
    first scalar), every key's run cut into blocks of 64"""
    nk = len(n_inputs)
    perm = [j for k in range(nk) for j, kj in enumerate(key_of) if kj == k]
    segs, blocks = [], []
    row = scalar = 0
    for k in range(nk):
        count = sum(1 for kj in key_of if kj == k)
        segs.append((row, count, scalar))
        for t in range(0, count, 64):
            blocks.append((k, row + t, min(64, count - t), scalar + t * n_inputs[k]))
        row += count
        scalar += count * n_inputs[k]
    return perm, segs, blocks
