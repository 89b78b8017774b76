"""`gadgets::sha256` (reference: src/gadgets/sha256.rs:13-270): SHA-256 and its compression function as circuits, and a ready
preimage circuit (the shape of the reference's crate example, src/lib.rs:16-126)."""

import hashlib

import numpy as np

from .boolean import AllocatedBit, Boolean
from .multieq import MultiEq
from .multipack import bytes_to_bits, compute_multipacking, pack_into_inputs
from .recorder import recorder_of
from .uint32 import UInt32

ROUND_CONSTANTS = [   # sha256.rs:13-22
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2,
]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]   # sha256.rs:25-27


def get_sha256_iv():
    """sha256.rs:76-78"""
    return [UInt32.constant(v) for v in IV]


def sha256_block_no_padding(cs, input_bits):
    """sha256.rs:29-45"""
    assert len(input_bits) == 512
    return [b for e in sha256_compression_function(cs, input_bits, get_sha256_iv()) for b in e.into_bits_be()]


def sha256(cs, input_bits):
    """sha256.rs:47-74"""
    assert len(input_bits) % 8 == 0
    padded = list(input_bits)
    plen = len(padded)
    padded.append(Boolean.constant(True))
    while (len(padded) + 64) % 512 != 0:
        padded.append(Boolean.constant(False))
    for i in range(63, -1, -1):
        padded.append(Boolean.constant((plen >> i) & 1))
    assert len(padded) % 512 == 0
    cur = get_sha256_iv()
    for lo in range(0, len(padded), 512):
        cur = sha256_compression_function(cs, padded[lo:lo + 512], cur)
    return [b for e in cur for b in e.into_bits_be()]


def _compute(maybe, cs, others):
    """sha256.rs:126-146: Maybe::Concrete(v) is a UInt32, Maybe::Deferred(vec) a list whose sum is still to be taken"""
    if isinstance(maybe, UInt32):
        return maybe
    return UInt32.addmany(cs, maybe + list(others))


def sha256_compression_function(cs, input_bits, current_hash_value):
    """sha256.rs:81-270"""
    assert len(input_bits) == 512 and len(current_hash_value) == 8
    w = [UInt32.from_bits_be(input_bits[lo:lo + 32]) for lo in range(0, 512, 32)]
    with MultiEq(cs) as cs:   # "we can save some constraints by combining some of the constraints in different u32 additions"
        for i in range(16, 64):
            s0 = w[i - 15].rotr(7)
            s0 = s0.xor(cs, w[i - 15].rotr(18))
            s0 = s0.xor(cs, w[i - 15].shr(3))
            s1 = w[i - 2].rotr(17)
            s1 = s1.xor(cs, w[i - 2].rotr(19))
            s1 = s1.xor(cs, w[i - 2].shr(10))
            w.append(UInt32.addmany(cs, [w[i - 16], s0, w[i - 7], s1]))
        assert len(w) == 64
        a, b, c, d, e, f, g, h = current_hash_value
        for i in range(64):
            new_e = _compute(e, cs, [])
            s1 = new_e.rotr(6)
            s1 = s1.xor(cs, new_e.rotr(11))
            s1 = s1.xor(cs, new_e.rotr(25))
            ch = UInt32.sha256_ch(cs, new_e, f, g)
            temp1 = [h, s1, ch, UInt32.constant(ROUND_CONSTANTS[i]), w[i]]
            new_a = _compute(a, cs, [])
            s0 = new_a.rotr(2)
            s0 = s0.xor(cs, new_a.rotr(13))
            s0 = s0.xor(cs, new_a.rotr(22))
            maj = UInt32.sha256_maj(cs, new_a, b, c)
            temp2 = [s0, maj]
            h, g, f = g, f, new_e
            e = temp1 + [d]          # Maybe::Deferred
            d, c, b = c, b, new_a
            a = temp1 + temp2        # Maybe::Deferred
        h0 = _compute(a, cs, [current_hash_value[0]])
        h1 = UInt32.addmany(cs, [current_hash_value[1], b])
        h2 = UInt32.addmany(cs, [current_hash_value[2], c])
        h3 = UInt32.addmany(cs, [current_hash_value[3], d])
        h4 = _compute(e, cs, [current_hash_value[4]])
        h5 = UInt32.addmany(cs, [current_hash_value[5], f])
        h6 = UInt32.addmany(cs, [current_hash_value[6], g])
        h7 = UInt32.addmany(cs, [current_hash_value[7], h])
    return [h0, h1, h2, h3, h4, h5, h6, h7]


class Sha256Preimage:
    """"I know n_bytes bytes whose SHA-256 (double=True: SHA-256 of SHA-256, as src/lib.rs:16-126) is this digest": the
    message bits are aux bits, the digest is exposed through pack_into_inputs (two inputs: 254 bits and 2 bits).

    The circuit is the callable itself; `with_message(m)` gives the copy that carries values.  For the word program the
    message is n_ext = ceil(n_bytes / 4) external words: word e holds bytes 4e .. 4e + 3 big-endian, absent bytes as zero
    (ext_from_messages)."""

    def __init__(self, n_bytes, double=False, message=None):
        assert message is None or len(message) == n_bytes
        self.n_bytes, self.double, self.message = n_bytes, double, message

    def with_message(self, message):
        return Sha256Preimage(self.n_bytes, self.double, bytes(message))

    @property
    def n_ext(self):
        return (self.n_bytes + 3) // 4

    def __call__(self, cs):
        r = recorder_of(cs)
        values = bytes_to_bits(self.message) if self.message is not None else [None] * (self.n_bytes * 8)
        bits, w = [], None
        for i, v in enumerate(values):
            if r is not None and i % 32 == 0:
                w = r.external()
            bits.append(Boolean.Is(AllocatedBit.alloc(cs, v, None if r is None else (w, 31 - i % 32, 0))))
        digest = sha256(cs, bits)
        if self.double:
            digest = sha256(cs, digest)
        pack_into_inputs(cs, digest)

    def ext_from_messages(self, messages):
        """k messages of n_bytes bytes -> [k, n_ext] uint32, what WordWitness.generate / generate_dev take"""
        out = np.zeros((len(messages), self.n_ext), dtype=np.uint32)
        for j, m in enumerate(messages):
            assert len(m) == self.n_bytes
            padded = bytes(m) + b"\0" * (4 * self.n_ext - self.n_bytes)
            out[j] = np.frombuffer(padded, dtype=">u4")
        return out

    def digest(self, message):
        d = hashlib.sha256(bytes(message)).digest()
        return hashlib.sha256(d).digest() if self.double else d

    def public_inputs(self, message):
        """the input assignment behind ONE: compute_multipacking of the digest's bits (multipack.rs:53-72)"""
        return compute_multipacking(bytes_to_bits(self.digest(message)))
