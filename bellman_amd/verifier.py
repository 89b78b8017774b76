"""groth16 verification on the device: prepare_verifying_key / verify_proof (groth16/src/verifier.rs:11-58) and
batch::Verifier (groth16/src/verifier/batch.rs), over include/bellman_hip.h's bh_groth16_* verifier entry points.

Public inputs and the batch's random z are Fr values given as Python ints (canonical; taken mod q).  Proofs are
`groth16.Proof` objects (affine Montgomery records: only the on-curve test is made) or the 192 bytes of `Proof::write`,
which are read on the device as Proof::read reads them (decompression, subgroup checks, no identity).  The pairing arithmetic runs in HIP kernels (csrc/pairing.hip);
there is no CPU path.
"""

import ctypes
import secrets

import numpy as np

from . import _lib
from ._abi import C
from .errors import (InvalidPoint, InvalidProof, InvalidVerifyingKey, PointAtInfinity, UnexpectedEof, check,
                     check_verification)

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
_CANONICAL = C.BH_SCALARS_CANONICAL


def _fr_bytes(vals):
    return b"".join((int(v) % Q).to_bytes(32, "little") for v in vals)


def _proof_bytes(proof):
    return np.concatenate([proof.a, proof.b, proof.c]).astype(np.uint64).tobytes()


class PreparedVerifyingKey:
    """groth16/src/lib.rs:400-409: the line coefficients of -gamma, -delta and beta in HBM, ic registered for the
    multiexp of the public inputs."""

    def __init__(self, worker, handle, n_inputs):
        self.worker, self._h, self.n_inputs = worker, handle, n_inputs

    @classmethod
    def from_elements(cls, worker, alpha_g1, beta_g2, gamma_g2, delta_g2, ic):
        lib = _lib.load()
        arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (alpha_g1, beta_g2, gamma_g2, delta_g2)]
        icv = np.ascontiguousarray(ic, dtype=np.uint64).reshape(-1, 12)
        h = ctypes.c_void_p()
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        check(lib.bh_groth16_prepare_verifying_key(worker.ctx, *[p(x) for x in arrs], p(icv), icv.shape[0], ctypes.byref(h)),
              "prepare_verifying_key")
        return cls(worker, h, icv.shape[0] - 1)

    def release(self):
        """must run before the worker's context is destroyed (its device memory lives in the context's pool); after
        that the handle is only dropped"""
        if self._h:
            if self.worker.ctx:
                _lib.load().bh_groth16_pvk_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def prepare_verifying_key(params):
    """prepare_verifying_key (groth16/src/verifier.rs:11-21) of generated or read `groth16.Parameters`"""
    lib = _lib.load()
    h = ctypes.c_void_p()
    check(lib.bh_groth16_pvk_from_params(params._h, ctypes.byref(h)), "prepare_verifying_key")
    return PreparedVerifyingKey(params.worker, h, lib.bh_groth16_pvk_num_inputs(h))


def _is_compressed(proof):
    return isinstance(proof, (bytes, bytearray, memoryview))


def verify_proof(pvk, proof, public_inputs):
    """verify_proof (groth16/src/verifier.rs:23-58): returns None, raises InvalidProof / InvalidVerifyingKey
    (or InvalidPoint for a proof point that is not on its curve).  `proof` may be the 192 bytes of Proof::write: they
    go through Proof.read first (InvalidPoint / PointAtInfinity / UnexpectedEof)."""
    if _is_compressed(proof):
        from .groth16 import Proof

        proof = Proof.read(pvk.worker, proof)
    raw = _proof_bytes(proof)
    ins = _fr_bytes(public_inputs)
    check_verification(_lib.load().bh_groth16_verify(pvk._h, raw, ins or None, len(public_inputs), _CANONICAL), "verify_proof")


def _verdict_error(code):
    """the exception Item.verify_single raises for a verdict code of bh_groth16_verify_each (None for BH_OK)"""
    if code == C.BH_OK:
        return None
    if code == C.BH_ERR_INVALID_PROOF:
        return InvalidProof()
    if code == C.BH_ERR_INVALID_POINT:
        return InvalidPoint("invalid G1/G2")
    if code == C.BH_ERR_POINT_AT_INFINITY:
        return PointAtInfinity("point at infinity")
    raise AssertionError("unexpected verdict code %d" % code)


_READ_VERDICTS = (C.BH_OK, C.BH_ERR_INVALID_POINT, C.BH_ERR_POINT_AT_INFINITY)   # what bh_proofs_read returns per proof


def _status_error(word):
    """the exception a status word of bh_proofs_read stands for (None for a readable proof)"""
    for e in range(3):   # the first bad element in the order a, b, c
        byte = (word >> (8 * e)) & 0xFF
        if byte & C.BH_PROOF_STATUS_INVALID:
            return InvalidPoint("invalid G1/G2")
        if byte & C.BH_PROOF_STATUS_IDENTITY:
            return PointAtInfinity("point at infinity")
    return None


def verify_each(pvk, items):
    """Item::verify_single (groth16/src/verifier/batch.rs:55-66) for every item, in one device call: a list with None for a
    good proof and, for a bad one, the exception instance Item.verify_single would raise (not raised).  Items are `Item`s or
    (proof, inputs) pairs; a proof is a groth16.Proof or the 192 bytes of Proof::write.  A batch of byte proofs only is read
    and judged on the device (bh_groth16_verify_each_compressed); in a mixed batch the byte items are read first, as
    Verifier._run does, and a read error becomes that item's entry.  Raises InvalidVerifyingKey before any work when an
    item's input count does not match the key."""
    items = [it if isinstance(it, Item) else Item(*it) for it in items]
    n_in = pvk.n_inputs
    if any(len(it.inputs) != n_in for it in items):
        raise InvalidVerifyingKey()
    n = len(items)
    if not n:
        return []
    lib = _lib.load()
    packed = [_is_compressed(it.proof) for it in items]
    if any(c and len(it.proof) != 192 for c, it in zip(packed, items)):
        raise UnexpectedEof("failed to fill whole buffer")
    ins = b"".join(_fr_bytes(it.inputs) for it in items)
    verdicts = (ctypes.c_int32 * n)()
    if all(packed):
        check_verification(lib.bh_groth16_verify_each_compressed(pvk._h, b"".join(bytes(it.proof) for it in items), n, ins or None,
                                                                 n_in, _CANONICAL, verdicts, None, None), "verify_each")
        return [_verdict_error(v) for v in verdicts]
    out = [None] * n
    decoded = {}
    where = [i for i, c in enumerate(packed) if c]
    if where:   # a mixed batch: the byte items are read first; the unreadable ones keep their read error
        from .groth16 import Proof

        raw = b"".join(bytes(items[i].proof) for i in where)
        recs = np.zeros((len(where), 48), dtype=np.uint64)
        status = (ctypes.c_uint32 * len(where))()
        rc = lib.bh_proofs_read(pvk.worker.ctx, raw, len(where), recs.ctypes.data_as(ctypes.c_void_p), status, None)
        if rc not in _READ_VERDICTS:
            check(rc, "Proof.read")
        for k, i in enumerate(where):
            out[i] = _status_error(status[k])
            decoded[i] = Proof(recs[k].copy())
    live = [i for i in range(n) if out[i] is None]
    if live:
        proofs = b"".join(_proof_bytes(decoded.get(i, items[i].proof)) for i in live)
        ins = b"".join(_fr_bytes(items[i].inputs) for i in live)
        verdicts = (ctypes.c_int32 * len(live))()
        check_verification(lib.bh_groth16_verify_each(pvk._h, proofs, len(live), ins or None, n_in, _CANONICAL, verdicts, None),
                           "verify_each")
        for i, v in zip(live, verdicts):
            out[i] = _verdict_error(v)
    return out


class Item:
    """batch::Item (groth16/src/verifier/batch.rs:37-66)"""

    def __init__(self, proof, inputs):
        self.proof, self.inputs = proof, list(inputs)

    def verify_single(self, pvk):
        return verify_proof(pvk, self.proof, self.inputs)


class Verifier:
    """batch::Verifier (groth16/src/verifier/batch.rs:68-275) for proofs of one verifying key"""

    def __init__(self):
        self.items = []

    def queue(self, item):
        """queue((proof, inputs)) or an Item; the proof is a groth16.Proof or the 192 bytes of Proof::write"""
        self.items.append(item if isinstance(item, Item) else Item(*item))

    def _run(self, pvk, zs):
        n_in = pvk.n_inputs
        # the reference checks every item's input count before any work (batch.rs:101-107)
        if any(len(it.inputs) != n_in for it in self.items):
            raise InvalidVerifyingKey()
        n = len(self.items)
        lib = _lib.load()
        ins = b"".join(_fr_bytes(it.inputs) for it in self.items)
        z = _fr_bytes(zs)
        packed = [_is_compressed(it.proof) for it in self.items]
        if n and all(packed):
            # every proof as written: read and verified in one call, the decoded proofs never leave the device
            if any(len(it.proof) != 192 for it in self.items):
                raise UnexpectedEof("failed to fill whole buffer")
            bad = ctypes.c_size_t(0)
            try:
                check_verification(lib.bh_groth16_batch_verify_compressed(pvk._h, b"".join(bytes(it.proof) for it in self.items), n,
                                                                          ins or None, n_in, _CANONICAL, z, ctypes.byref(bad)),
                                   "batch verify")
            except IOError as e:
                e.index = bad.value
                raise
            return
        if any(packed):   # a mixed batch: the byte items are read first
            from .groth16 import read_proofs

            where = [i for i, c in enumerate(packed) if c]
            if any(len(self.items[i].proof) != 192 for i in where):
                raise UnexpectedEof("failed to fill whole buffer")
            try:
                read = read_proofs(pvk.worker, b"".join(bytes(self.items[i].proof) for i in where))
            except IOError as e:
                e.index = where[e.index]
                raise
            decoded = dict(zip(where, read))
        else:
            decoded = {}
        proofs = b"".join(_proof_bytes(decoded.get(i, it.proof)) for i, it in enumerate(self.items))
        check_verification(lib.bh_groth16_batch_verify(pvk._h, proofs or None, n, ins or None, n_in, _CANONICAL,
                                                               z or None), "batch verify")

    def verify(self, rng, pvk):
        """Verifier::verify(rng, vk) (batch.rs:93-192): z_j drawn from rng (randrange / getrandbits), redrawn while 0"""
        zs = []
        for _ in self.items:
            z = 0
            while z == 0:
                z = rng.randrange(Q) if hasattr(rng, "randrange") else rng.getrandbits(256) % Q
            zs.append(z)
        return self._run(pvk, zs)

    def verify_multicore(self, pvk):
        """Verifier::verify_multicore(vk) (batch.rs:194-275): z_j from the operating system's CSPRNG"""
        zs = []
        for _ in self.items:
            z = 0
            while z == 0:
                z = secrets.randbelow(Q)
            zs.append(z)
        return self._run(pvk, zs)

    def verify_each(self, pvk):
        """per-item verdicts of the queued items (module-level verify_each): None or the exception verify_single would raise"""
        return verify_each(pvk, self.items)

    def find_invalid(self, rng, pvk):
        """the fallback batch.rs:55-66 describes, as one call: [] when the batch check passes, else the indices of the items
        whose own verification fails"""
        try:
            self.verify(rng, pvk)
            return []
        except (InvalidProof, IOError):
            pass
        return [i for i, e in enumerate(self.verify_each(pvk)) if e is not None]


# ---- proofs of several verifying keys in one call (bh_pvk_set, bh_groth16_*_keys) ------------------------------------------
class KeySet:
    """1 .. 64 prepared keys of one worker, addressed by position: proofs of all of them are judged in one device call
    (verify_each_keys, MultiVerifier).  The set keeps its keys alive; release it before the worker's context goes."""

    def __init__(self, pvks):
        self.pvks = list(pvks)
        lib = _lib.load()
        handles = (ctypes.c_void_p * max(len(self.pvks), 1))(*[k._h for k in self.pvks])
        h = ctypes.c_void_p()
        check(lib.bh_groth16_pvk_set_create(handles, len(self.pvks), ctypes.byref(h)), "KeySet")
        self._h = h
        self.worker = self.pvks[0].worker

    def __len__(self):
        return len(self.pvks)

    def n_inputs(self, key_index):
        return self.pvks[key_index].n_inputs

    def release(self):
        if self._h:
            if self.worker.ctx:
                _lib.load().bh_groth16_pvk_set_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class _KeyedItem:
    def __init__(self, key_index, proof, inputs):
        self.key_index, self.proof, self.inputs = int(key_index), proof, list(inputs)


def _keyed(items):
    out = []
    for it in items:
        if isinstance(it, _KeyedItem):
            out.append(it)
        else:
            k, proof, inputs = it
            out.append(_KeyedItem(k, proof, inputs))
    return out


def _check_keyed(keyset, items):
    """before any work: every item names a key of the set (IndexError) and carries that key's input count"""
    for it in items:
        if not 0 <= it.key_index < len(keyset):
            raise IndexError("key index %d outside a set of %d keys" % (it.key_index, len(keyset)))
    if any(len(it.inputs) != keyset.n_inputs(it.key_index) for it in items):
        raise InvalidVerifyingKey()


def _key_of(items):
    return (ctypes.c_uint32 * max(len(items), 1))(*[it.key_index for it in items])


def verify_each_keys(keyset, items):
    """verify_each over proofs of several keys: items are (key_index, proof, inputs); the result holds, item by item, None
    or the exception Item(proof, inputs).verify_single(keyset.pvks[key_index]) would raise.  Byte and Proof items mix as in
    verify_each.  Raises InvalidVerifyingKey before any work when an item's input count is not its key's."""
    items = _keyed(items)
    _check_keyed(keyset, items)
    n = len(items)
    if not n:
        return []
    lib = _lib.load()
    packed = [_is_compressed(it.proof) for it in items]
    if any(c and len(it.proof) != 192 for c, it in zip(packed, items)):
        raise UnexpectedEof("failed to fill whole buffer")
    if all(packed):
        ins = b"".join(_fr_bytes(it.inputs) for it in items)
        verdicts = (ctypes.c_int32 * n)()
        check_verification(lib.bh_groth16_verify_each_keys_compressed(
            keyset._h, _key_of(items), b"".join(bytes(it.proof) for it in items), n, ins or None, len(ins) // 32, _CANONICAL,
            verdicts, None, None), "verify_each_keys")
        return [_verdict_error(v) for v in verdicts]
    out = [None] * n
    decoded = {}
    where = [i for i, c in enumerate(packed) if c]
    if where:   # a mixed batch: the byte items are read first; the unreadable ones keep their read error
        from .groth16 import Proof

        raw = b"".join(bytes(items[i].proof) for i in where)
        recs = np.zeros((len(where), 48), dtype=np.uint64)
        status = (ctypes.c_uint32 * len(where))()
        rc = lib.bh_proofs_read(keyset.worker.ctx, raw, len(where), recs.ctypes.data_as(ctypes.c_void_p), status, None)
        if rc not in _READ_VERDICTS:
            check(rc, "Proof.read")
        for k, i in enumerate(where):
            out[i] = _status_error(status[k])
            decoded[i] = Proof(recs[k].copy())
    live = [i for i in range(n) if out[i] is None]
    if live:
        sub = [items[i] for i in live]
        proofs = b"".join(_proof_bytes(decoded.get(i, items[i].proof)) for i in live)
        ins = b"".join(_fr_bytes(it.inputs) for it in sub)
        verdicts = (ctypes.c_int32 * len(live))()
        check_verification(lib.bh_groth16_verify_each_keys(keyset._h, _key_of(sub), proofs, len(live), ins or None, len(ins) // 32,
                                                           _CANONICAL, verdicts, None), "verify_each_keys")
        for i, v in zip(live, verdicts):
            out[i] = _verdict_error(v)
    return out


class MultiVerifier:
    """batch::Verifier for proofs of several verifying keys: Verifier, method for method, over a KeySet.  One batch check
    covers all keys (one product, one final exponentiation)."""

    def __init__(self):
        self.items = []

    def queue(self, key_index, item):
        """queue(key_index, (proof, inputs)) or an Item; the proof is a groth16.Proof or the 192 bytes of Proof::write"""
        item = item if isinstance(item, Item) else Item(*item)
        self.items.append(_KeyedItem(key_index, item.proof, item.inputs))

    def _run(self, keyset, zs):
        _check_keyed(keyset, self.items)   # the reference checks every item's input count before any work (batch.rs:101-107)
        n = len(self.items)
        lib = _lib.load()
        ins = b"".join(_fr_bytes(it.inputs) for it in self.items)
        z = _fr_bytes(zs)
        key_of = _key_of(self.items)
        packed = [_is_compressed(it.proof) for it in self.items]
        if n and all(packed):
            if any(len(it.proof) != 192 for it in self.items):
                raise UnexpectedEof("failed to fill whole buffer")
            bad = ctypes.c_size_t(0)
            try:
                check_verification(lib.bh_groth16_batch_verify_keys_compressed(
                    keyset._h, key_of, b"".join(bytes(it.proof) for it in self.items), n, ins or None, len(ins) // 32, _CANONICAL,
                    z, ctypes.byref(bad)), "batch verify")
            except IOError as e:
                e.index = bad.value
                raise
            return
        if any(packed):   # a mixed batch: the byte items are read first
            from .groth16 import read_proofs

            where = [i for i, c in enumerate(packed) if c]
            if any(len(self.items[i].proof) != 192 for i in where):
                raise UnexpectedEof("failed to fill whole buffer")
            try:
                read = read_proofs(keyset.worker, b"".join(bytes(self.items[i].proof) for i in where))
            except IOError as e:
                e.index = where[e.index]
                raise
            decoded = dict(zip(where, read))
        else:
            decoded = {}
        proofs = b"".join(_proof_bytes(decoded.get(i, it.proof)) for i, it in enumerate(self.items))
        check_verification(lib.bh_groth16_batch_verify_keys(keyset._h, key_of, proofs or None, n, ins or None, len(ins) // 32,
                                                            _CANONICAL, z or None), "batch verify")

    def verify(self, rng, keyset):
        """Verifier.verify over the set: z_j drawn from rng (randrange / getrandbits), redrawn while 0"""
        zs = []
        for _ in self.items:
            z = 0
            while z == 0:
                z = rng.randrange(Q) if hasattr(rng, "randrange") else rng.getrandbits(256) % Q
            zs.append(z)
        return self._run(keyset, zs)

    def verify_multicore(self, keyset):
        """Verifier.verify_multicore over the set: z_j from the operating system's CSPRNG"""
        zs = []
        for _ in self.items:
            z = 0
            while z == 0:
                z = secrets.randbelow(Q)
            zs.append(z)
        return self._run(keyset, zs)

    def verify_each(self, keyset):
        """per-item verdicts of the queued items (verify_each_keys)"""
        return verify_each_keys(keyset, self.items)

    def find_invalid(self, rng, keyset):
        """[] when the batch check passes, else the indices of the items whose own verification fails"""
        try:
            self.verify(rng, keyset)
            return []
        except (InvalidProof, IOError):
            pass
        return [i for i, e in enumerate(self.verify_each(keyset)) if e is not None]
