"""Batches for the point-cache tests (tests/test_gpu_point_cache*.py), built
once per process, each with the C oracle's validity vector."""
import functools
import json
import os
import random

import numpy as np

import oracle_c as C
from tendermint_amd.testing.factory import (Ed25519Signer, key_seed, make_c2_batch, make_commit_batch,
                                            undecodable_encodings)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
N = 1024


class Case:
    def __init__(self, ents):
        self.pk, self.sig, self.msg, self.off = C.pack(ents)
        self.n = len(ents)
        _, self.ref = C.ed25519_verify_packed(self.pk, self.sig, self.msg, self.off, threads=4)
        keys = [e[0] for e in ents]
        self.decodable = np.array([decodable(k) for k in keys], bool)
        self.keys = keys


def decodable(key: bytes) -> bool:
    """ZIP-215: x^2 = (y^2 - 1) / (d y^2 + 1) has a root (y taken mod p)."""
    y = (int.from_bytes(key, "little") & ((1 << 255) - 1)) % P
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    r = u * pow(v, P - 2, P) % P
    return r == 0 or pow(r, (P - 1) // 2, P) == 1


def _flip255(pk: bytes) -> bytes:
    return pk[:31] + bytes([pk[31] ^ 0x80])


@functools.lru_cache(None)
def edge_case() -> Case:
    """1,024 entries: the 196 small-order (A, R) pairs (non-canonical y, x = 0
    with the sign bit set among them), a C2-shaped slice (valid, bit-flipped,
    S + l, undecodable), undecodable keys on honest signatures (one three
    times), pairs of keys that differ only in bit 255, one key signing many
    messages, one entry repeated, honest fill."""
    g = json.load(open(os.path.join(REPO, "tests", "golden", "zip215_small_order.json")))
    msg0 = bytes.fromhex(g["msg"])
    ents = [(bytes.fromhex(a), msg0, bytes.fromhex(r) + bytes(32)) for a, r in g["pairs_all_valid_with_S0"]]
    c2 = make_c2_batch(560, seed=61, edge_scale=4.0)
    ents += [c2.entry(i) for i in range(c2.n)]
    hon = make_commit_batch(300, seed=62)
    undec = undecodable_encodings(24, random.Random(9))
    for j, u in enumerate(undec):
        ents.append((u,) + hon.entry(j)[1:])
    ents += [(undec[0],) + hon.entry(30)[1:]] * 2
    for j in range(40, 80):
        pk, msg, sig = hon.entry(j)
        ents += [(pk, msg, sig), (_flip255(pk), msg, sig)]
    s = Ed25519Signer(key_seed(7, "pc"))
    for j in range(12):
        m = hon.entry(100 + j)[1]
        ents.append((s.public_key, m, s.sign(m)))
    ents += [hon.entry(120)] * 6
    ents += [hon.entry(130 + j) for j in range(N - len(ents))]
    assert len(ents) == N
    return Case(ents)


@functools.lru_cache(None)
def c2_case(seed: int) -> Case:
    b = make_c2_batch(N, seed=seed, edge_scale=5.0)
    return Case([b.entry(i) for i in range(b.n)])


@functools.lru_cache(None)
def commit_case() -> Case:
    """Honest commit signatures with every 37th signature's R bit-flipped."""
    b = make_commit_batch(N, seed=64)
    ents = []
    for i in range(b.n):
        pk, msg, sig = b.entry(i)
        if i % 37 == 5:
            sig = bytes([sig[0] ^ 4]) + sig[1:]
        ents.append((pk, msg, sig))
    return Case(ents)


@functools.lru_cache(None)
def plain_case() -> Case:
    """No key with x = 0 (for the poisoning tests: a negated or zeroed x is
    then never the right one): C2-shaped honest / bit-flipped / undecodable
    entries without the small-order ones."""
    b = make_c2_batch(1400, seed=65, edge_scale=5.0)
    ents = [b.entry(i) for i in range(b.n) if b.kinds[i] not in ("small_order", "noncanonical_y", "neg_zero")][:N]
    assert len(ents) == N
    return Case(ents)
