"""The point cache's host-checkable half (tendermint_amd/csrc/point_cache.h,
compiled with limb-bound assertions into tests/native/pcache): the checked
load against ge_decode_zip215 over the golden edge encodings and 10,000
random keys, the table on the host, and the steady-state miss share of a
10,000-key validator set at the default capacity.  No GPU."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tendermint_amd.testing.factory import make_c2_batch, undecodable_encodings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libpcachecheck.so")
DEFAULT_SLOTS = 1 << 21  # kPointCacheSlots (tmverify_runtime.cpp)


@pytest.fixture(scope="module")
def P():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "pcache")], check=True)
    L = ctypes.CDLL(SO)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.pcachecheck_hash.argtypes = [u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.pcachecheck_round_slots.argtypes = [ctypes.c_uint64]
    L.pcachecheck_round_slots.restype = ctypes.c_uint32
    L.pcachecheck_checked_load.argtypes = [u8p, ctypes.c_uint32, u8p]
    L.pcachecheck_checked_load.restype = ctypes.c_int64
    L.pcachecheck_table.argtypes = [u8p, ctypes.c_uint32, ctypes.c_uint32, u8p]
    L.pcachecheck_table.restype = ctypes.c_int64
    return L


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _edge_keys():
    g = json.load(open(os.path.join(REPO, "tests", "golden", "zip215_small_order.json")))
    enc = [bytes.fromhex(e) for e in g["encodings"]]
    undec = undecodable_encodings(16, random.Random(5))
    both = [bytes(u[:31]) + bytes([u[31] ^ 0x80]) for u in undec]
    return enc + undec + both


def test_checked_load_matches_decode(P):
    rng = np.random.default_rng(11)
    keys = np.concatenate([np.frombuffer(b"".join(_edge_keys()), np.uint8),
                           rng.integers(0, 256, 32 * 10_000, dtype=np.uint8)])
    n = len(keys) // 32
    dec = np.zeros(n, np.uint8)
    good = P.pcachecheck_checked_load(_u8(keys), n, _u8(dec))
    assert good > 0, good
    assert dec[:14].all()              # the 14 small-order encodings decode (non-canonical y, x = 0 with the sign bit)
    assert not dec[14:14 + 32].any()   # the undecodable ones, with either sign bit
    assert 4000 < int(dec[46:].sum()) < 6000  # about half of random encodings are on the curve


def test_table_on_host(P):
    rng = np.random.default_rng(12)
    keys = np.concatenate([np.frombuffer(b"".join(_edge_keys()), np.uint8),
                           rng.integers(0, 256, 32 * 2000, dtype=np.uint8)])
    n = len(keys) // 32
    dec = np.zeros(n, np.uint8)
    assert P.pcachecheck_checked_load(_u8(keys), n, _u8(dec)) > 0
    hits = np.zeros(n, np.uint8)
    # roomy table: every decodable key but the few sharing a slot is served, no undecodable one is
    served = P.pcachecheck_table(_u8(keys), n, 1 << 16, _u8(hits))
    assert served > 0 and not hits[dec == 0].any()
    assert int(dec.sum()) - served <= 2 * int(dec.sum()) ** 2 // (1 << 16) + 4
    # one bucket: at most two keys survive, and what is served is still exact
    served = P.pcachecheck_table(_u8(keys), n, 2, _u8(hits))
    assert 1 <= served <= 2


def test_round_slots(P):
    assert [P.pcachecheck_round_slots(x) for x in (0, 1, 2, 3, 4, 1000, 1 << 21, (1 << 21) + 5, 1 << 40)] == \
        [0, 2, 2, 2, 4, 512, 1 << 21, 1 << 21, 1 << 24]


def test_default_capacity_miss_share(P):
    """A key has one slot (bucket and way are hash bits), so in the steady
    state the keys that share a slot with another key evict each other: their
    share among the factory's 10,000 validator keys must stay below 1 % at
    the default capacity."""
    b = make_c2_batch(10_000)
    keys = np.unique(np.ascontiguousarray(b.pk).reshape(-1, 32), axis=0)
    assert len(keys) > 9_800
    flat = np.ascontiguousarray(keys).reshape(-1)
    h = np.zeros(len(keys), np.uint32)
    P.pcachecheck_hash(_u8(flat), len(keys), h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    slot = (h & np.uint32(DEFAULT_SLOTS // 2 - 1)).astype(np.int64) * 2 + (h >> np.uint32(31))
    _, counts = np.unique(slot, return_counts=True)
    colliding = int(counts[counts > 1].sum())
    share = colliding / len(keys)
    print(f"point cache: {len(keys)} keys, {DEFAULT_SLOTS} slots, {colliding} share a slot ({100 * share:.2f} %)")
    assert share < 0.01
