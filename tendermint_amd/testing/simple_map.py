"""Valid fixtures for tmv_proof_ops_verify / tmv_merkle_value_ops (TEST SUPPORT,
never part of the product path): maps of (key, value) pairs as the reference's
value ops prove them.

A map's pairs, sorted by key, become the KV leaves
    uvarint(len key) || key || uvarint(32) || SHA-256(value)
(ValueOp.Run, crypto/merkle/proof_value.go:77-98) of one RFC 6962 tree; the
proof of a pair is the "simple:v" op (key, merkle.Proof of its leaf).  A
multistore nests maps: the root of an inner map is the value of a key of the
next map outwards, which is why ops chain at all (two- and three-op proofs).
Roots and proofs come from a proof generator `proofs(items) -> (root,
[proof...])` with proof.total / index / leaf_hash / aunts: by default the
hashlib one below; the tests pass their restatement of ProofsFromByteSlices.
"""
from __future__ import annotations

import hashlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from .. import host as H


def uvarint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def kv_leaf(key: bytes, value: bytes) -> bytes:
    """The bytes ValueOp.Run hashes as a leaf for (key, value)."""
    return uvarint(len(key)) + key + uvarint(32) + hashlib.sha256(value).digest()


def _leaf(b: bytes) -> bytes:
    return hashlib.sha256(b"\x00" + b).digest()


def _inner(l: bytes, r: bytes) -> bytes:
    return hashlib.sha256(b"\x01" + l + r).digest()


def _tree(hashes: Sequence[bytes]) -> Tuple[bytes, List[List[bytes]]]:
    """(root, aunts of every leaf, leaf sibling first) of the split-point tree."""
    n = len(hashes)
    if n == 1:
        return hashes[0], [[]]
    k = 1
    while k * 2 < n:
        k *= 2
    lr, la = _tree(hashes[:k])
    rr, ra = _tree(hashes[k:])
    return _inner(lr, rr), [a + [rr] for a in la] + [a + [lr] for a in ra]


def hashlib_proofs(items: Sequence[bytes]):
    """merkle.ProofsFromByteSlices over hashlib: (root, [host.Proof])."""
    if not items:
        return hashlib.sha256(b"").digest(), []
    hashes = [_leaf(x) for x in items]
    root, aunts = _tree(hashes)
    return root, [H.Proof(len(items), i, hashes[i], aunts[i]) for i in range(len(items))]


class SimpleMap:
    """One map: .root, and .op(key) = the value op proving that key's pair."""

    def __init__(self, pairs: Dict[bytes, bytes], proofs: Optional[Callable] = None):
        self.keys = sorted(pairs)
        self.pairs = dict(pairs)
        root, prs = (proofs or hashlib_proofs)([kv_leaf(k, pairs[k]) for k in self.keys])
        self.root = root
        self._proofs = [H.Proof(p.total, p.index, p.leaf_hash, list(p.aunts)) for p in prs]

    def op(self, key: bytes) -> H.ValueOp:
        return H.ValueOp(key, self._proofs[self.keys.index(key)])


def nested(levels: Sequence[Tuple[Dict[bytes, bytes], bytes]], proofs: Optional[Callable] = None) -> H.ProofOpsItem:
    """A chain of len(levels) ops.  levels[0] = (pairs, key): the innermost map
    and the key queried in it; levels[j] = (pairs, key) for j > 0: the map one
    step outwards, in which `key` gets the root of the map before as its value.
    The item's value is levels[0]'s pair, its root the outermost map's, its
    keys the key path (outermost first, as KeyPathToKeys returns it)."""
    value = levels[0][0][levels[0][1]]
    ops, carried = [], None
    for j, (pairs, key) in enumerate(levels):
        pairs = dict(pairs)
        if j > 0:
            pairs[key] = carried
        m = SimpleMap(pairs, proofs)
        ops.append(m.op(key))
        carried = m.root
    return H.ProofOpsItem(ops, carried, [key for _, key in reversed(levels)], value)
