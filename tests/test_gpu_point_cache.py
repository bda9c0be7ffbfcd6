"""The point cache (tendermint_amd/csrc/point_cache.h): uncached ed25519
batch-equation launches probe a per-device table of decoded public keys and
decode only what the probe could not serve.  A hit is checked, never trusted,
so every vector below must equal the C oracle's whatever the table holds --
cold, warm, one bucket shared by alternating or concurrent batches, off --
and the counters must show that the table is really used.  The launches here
are 1,024 entries; tmv_internal_option "point_cache_min" lowers the entry
threshold (120,000 in the product) for them."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tendermint_amd import _native as N

import point_cache_cases as K

pytestmark = pytest.mark.gpu

ED, BEQ = N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _set_min(n):
    L = N.lib()
    L.tmv_internal_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    assert L.tmv_internal_option(b"point_cache_min", int(n)) == 0


@pytest.fixture
def open_ctx(monkeypatch):
    """open_ctx(slots, min_n) -> a context whose device table has that capacity."""
    made = []

    def make(slots, min_n=512):
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        if slots is None:
            monkeypatch.delenv("TMV_POINT_CACHE_SLOTS", raising=False)
        else:
            monkeypatch.setenv("TMV_POINT_CACHE_SLOTS", str(slots))
        _set_min(min_n)
        c = N.Context(1)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()
    _set_min(0)


def _verify(ctx, case):
    ok, st = ctx.verify_batch_ex(ED, BEQ, case.pk, case.sig, case.msg, case.off)
    return np.asarray(st).astype(np.uint8)


def _delta(ctx, before):
    s = ctx.point_cache_stats()
    return s["hits"] - before["hits"], s["misses"] - before["misses"]


def _no_shared_slot(case, slots):
    """The test's own precondition for exact counters: no two distinct
    decodable keys of the batch share a slot of the table."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "pcache")], check=True)
    H = ctypes.CDLL(os.path.join(REPO, "oracle", "_build", "libpcachecheck.so"))
    H.pcachecheck_slot_word.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    H.pcachecheck_slot_word.restype = ctypes.c_uint64
    keys = {k for k, d in zip(case.keys, case.decodable) if d}
    return len({H.pcachecheck_slot_word(k, slots) for k in keys}) == len(keys)


def test_edge_keys_cold_and_warm(open_ctx):
    case = K.edge_case()
    undec = int((~case.decodable).sum())
    assert undec >= 26 and case.ref.any() and not case.ref.all()
    slots = 1 << 21
    assert _no_shared_slot(case, slots)
    ctx = open_ctx(slots)
    assert ctx.point_cache_stats() == {"hits": 0, "misses": 0, "slots": slots}
    s0 = ctx.point_cache_stats()
    assert np.array_equal(_verify(ctx, case), case.ref)       # cold: every key is decoded
    assert _delta(ctx, s0) == (0, case.n)
    for _ in range(2):                                        # warm, warm again
        s0 = ctx.point_cache_stats()
        assert np.array_equal(_verify(ctx, case), case.ref)
        # exactly the undecodable keys miss (they are never inserted); the table serves the rest
        assert _delta(ctx, s0) == (case.n - undec, undec)


def test_tiny_table_alternating_batches(open_ctx):
    ctx = open_ctx(2)  # one bucket
    assert ctx.point_cache_stats()["slots"] == 2
    a, b = K.edge_case(), K.c2_case(63)
    for r in range(6):
        case = b if r & 1 else a
        assert np.array_equal(_verify(ctx, case), case.ref), r
    s = ctx.point_cache_stats()
    assert s["hits"] + s["misses"] == 6 * K.N and s["misses"] > 5 * K.N


@pytest.mark.parametrize("slots", [2, 4096])
def test_concurrent_launches(open_ctx, slots):
    """Four host-buffer calls at once (each claims its own lane, so four
    streams share the table) for a few rounds."""
    ctx = open_ctx(slots)
    cases = [K.edge_case(), K.c2_case(63), K.commit_case(), K.c2_case(66)]
    for _ in range(3):
        with ThreadPoolExecutor(4) as ex:
            got = list(ex.map(lambda c: _verify(ctx, c), cases))
        for g, c in zip(got, cases):
            assert np.array_equal(g, c.ref)
    s = ctx.point_cache_stats()
    assert s["hits"] + s["misses"] == 3 * 4 * K.N


def test_disabled_and_below_threshold(open_ctx):
    case = K.edge_case()
    ctx = open_ctx(0)
    for _ in range(2):
        assert np.array_equal(_verify(ctx, case), case.ref)
    assert ctx.point_cache_stats() == {"hits": 0, "misses": 0, "slots": 0}
    ctx2 = open_ctx(4096, min_n=K.N + 1)  # the launch is one entry short of the threshold
    for _ in range(2):
        assert np.array_equal(_verify(ctx2, case), case.ref)
    assert ctx2.point_cache_stats() == {"hits": 0, "misses": 0, "slots": 4096}
    _set_min(0)  # the product's threshold: 1,024 entries are far below it
    for _ in range(2):
        assert np.array_equal(_verify(ctx2, case), case.ref)
    assert ctx2.point_cache_stats() == {"hits": 0, "misses": 0, "slots": 4096}
