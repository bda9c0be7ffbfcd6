"""csrc/host/key_order.h (the key order of a key-merged chunk: the per-chunk
histogram, the stable counting sort by key slot, the runs cut at group edges,
the rule for when merging is worth it, and where the run arrays sit) through
tests/native/keyorder, against a restatement in numpy, and the same header
under ASan + UBSan as a stand-alone program.  No GPU; nothing sanitized is
loaded into this interpreter."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libkeyordercheck.so")
UNWRITTEN = 0xEEEEEEEE
U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    u32 = ctypes.c_uint32
    L.ko_sort_chunks.restype = u32
    L.ko_histogram.restype = ctypes.c_int64
    L.ko_histogram.argtypes = [U32P, u32, u32, U32P]
    L.ko_merge_worth.argtypes = [u32, u32, u32]
    L.ko_region.restype = None
    L.ko_region.argtypes = [u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.ko_order_runs.restype = ctypes.c_int64
    L.ko_order_runs.argtypes = [U32P, u32, u32, u32, u32, U32P, U32P, U32P, U32P, U32P]
    return L


def _p(a):
    return a.ctypes.data_as(U32P)


def _restated(slots, m):
    """order: the stable sort by slot.  A run starts at work slot 0, at every multiple of m and where the key
    changes; group g's runs start at the first run at or behind work slot g * m."""
    n = len(slots)
    G = (n + m - 1) // m
    order = np.argsort(slots, kind="stable").astype(np.uint32)
    keys = slots[order]
    e = np.arange(n)
    starts = np.flatnonzero((e % m == 0) | (keys != np.roll(keys, 1)) | (e == 0))
    lo = np.append(starts, n).astype(np.uint32)
    group_run0 = np.searchsorted(starts, np.minimum(np.arange(G + 1) * m, n), side="left").astype(np.uint32)
    return order, lo, keys[starts].astype(np.uint32), group_run0


def _run(lib, slots, kc, m_log2):
    slots = np.ascontiguousarray(slots, np.uint32)
    n, m = len(slots), 1 << m_log2
    G = (n + m - 1) // m
    distinct = len(np.unique(slots))
    run_cap = distinct + G
    order, lo, slot, g0 = (np.zeros(k, np.uint32) for k in (n, run_cap + 1, run_cap, G + 1))
    d = ctypes.c_uint32(0)
    n_runs = lib.ko_order_runs(_p(slots), n, kc, m_log2, G, ctypes.byref(d), _p(order), _p(lo), _p(slot), _p(g0))
    assert n_runs >= 0, "a guard word around the output arrays was overwritten"
    assert d.value == distinct
    return n_runs, run_cap, order, lo, slot, g0


def _check(lib, slots, kc, m_log2):
    slots = np.asarray(slots, np.uint32)
    n, m = len(slots), 1 << m_log2
    G = (n + m - 1) // m
    n_runs, run_cap, order, lo, slot, g0 = _run(lib, slots, kc, m_log2)
    r_order, r_lo, r_slot, r_g0 = _restated(slots, m)
    assert n_runs == len(r_slot) and n_runs <= run_cap
    assert np.array_equal(order, r_order)
    assert np.array_equal(lo[:n_runs + 1], r_lo) and lo[n_runs] == n
    assert np.array_equal(slot[:n_runs], r_slot)
    assert np.array_equal(g0, r_g0) and g0[G] == n_runs
    # the properties the kernels rely on, stated directly
    assert np.array_equal(np.sort(order), np.arange(n))
    assert (np.diff(lo[:n_runs + 1].astype(np.int64)) > 0).all()
    for r in range(n_runs):
        a, b = int(lo[r]), int(lo[r + 1])
        assert a // m == (b - 1) // m, "a run lies in one group"
        assert (slots[order[a:b]] == slot[r]).all(), "a run holds one key"
    assert (np.diff(g0.astype(np.int64)) >= 0).all()
    # nothing behind the runs there are: the rest of lo and slot was left alone
    assert (lo[n_runs + 1:] == UNWRITTEN).all() and (slot[n_runs:] == UNWRITTEN).all()
    return n_runs, g0


@pytest.mark.parametrize("m_log2", [6, 7])
def test_order_and_runs_equal_the_restatement(lib, m_log2):
    m = 1 << m_log2
    rng = np.random.default_rng(70 + m_log2)
    for n in (1, 2, 15, 16, 17, m - 1, m, m + 1, 3 * m + 5):
        # kc = 1; n < 16 leaves counting-sort chunks empty
        assert _check(lib, np.zeros(n), 1, m_log2)[0] == (n + m - 1) // m
        # one key on every entry: cut at every edge, one run per group
        n_runs, g0 = _check(lib, np.full(n, 4), 9, m_log2)
        assert n_runs == (n + m - 1) // m and np.array_equal(g0, np.arange(len(g0)))
        # all keys distinct (in reverse, so the order is no identity), with and without unused slots behind them
        assert _check(lib, np.arange(n)[::-1], n, m_log2)[0] == n
        _check(lib, np.arange(n)[::-1], n + 9, m_log2)
        # slot ids with gaps: keys of the cache that no entry uses
        _check(lib, 3 + 7 * (np.arange(n) % 5), 40, m_log2)
        _check(lib, np.arange(n) % 3, 3, m_log2)
        _check(lib, rng.integers(0, 11, n), 11, m_log2)


@pytest.mark.parametrize("m_log2", [6, 7])
def test_segments_at_group_edges(lib, m_log2):
    m = 1 << m_log2
    # key 1 ends exactly on the first group edge... and key 4 starts exactly on it
    n_runs, g0 = _check(lib, np.repeat([1, 4], [m, 5]), 6, m_log2)
    assert n_runs == 2 and list(g0) == [0, 1, 2]
    # key 6 covers groups 1..3 from inside group 0: groups 1 and 2 hold no start of a key, only the cut
    slots = np.repeat([1, 6, 9], [m - 10, 3 * m + 1, 7])
    n_runs, g0 = _check(lib, slots, 10, m_log2)
    assert n_runs == 6 and list(g0) == [0, 2, 3, 4, 6]
    _check(lib, slots[::-1].copy(), 10, m_log2)
    # one key on every entry of three whole groups: n_runs = G
    assert _check(lib, np.full(3 * m, 2), 3, m_log2)[0] == 3


@pytest.mark.parametrize("m_log2", [6, 7])
def test_a_group_without_a_run_start_repeats_group_run0(lib, m_log2):
    """G is the caller's: with more groups than ceil(n / m) (the allocation of a launch may round up), the groups
    behind the entries hold no run, and group_run0 repeats n_runs for them.  Here the entries fill one group and
    five slots of the next; G is two more than that."""
    m = 1 << m_log2
    slots = np.repeat([0, 1], [m - 2, 7]).astype(np.uint32)
    n, G, kc = len(slots), 4, 2
    order, lo, slot, g0 = (np.zeros(k, np.uint32) for k in (n, 2 + G + 1, 2 + G, G + 1))
    d = ctypes.c_uint32(0)
    n_runs = lib.ko_order_runs(_p(slots), n, kc, m_log2, G, ctypes.byref(d), _p(order), _p(lo), _p(slot), _p(g0))
    assert n_runs == 3 and d.value == 2
    assert list(g0) == [0, 2, 3, 3, 3] and list(lo[:4]) == [0, m - 2, m, n] and list(slot[:3]) == [0, 1, 1]


def test_histogram(lib):
    rng = np.random.default_rng(71)
    chunks = lib.ko_sort_chunks()
    assert chunks == 16
    for n, kc in ((1, 1), (7, 3), (16, 5), (1000, 37), (129, 200)):
        slots = rng.integers(0, kc, n).astype(np.uint32)
        hist = np.zeros(chunks * kc, np.uint32)
        distinct = lib.ko_histogram(_p(slots), n, kc, _p(hist))
        assert distinct == len(np.unique(slots))
        bounds = [n * c // chunks for c in range(chunks + 1)]
        want = np.stack([np.bincount(slots[bounds[c]:bounds[c + 1]], minlength=kc) for c in range(chunks)])
        assert np.array_equal(hist.reshape(chunks, kc), want)


def test_merge_rule_at_its_boundary(lib):
    """distinct + G <= n / 2 (integer division)."""
    for n in (64, 65, 129, 200, 1 << 20):
        for G in (1, 2, n // 4):
            d = n // 2 - G
            assert lib.ko_merge_worth(d, G, n) == 1       # distinct + G == n / 2
            assert lib.ko_merge_worth(d + 1, G, n) == 0   # one above
    assert lib.ko_merge_worth(1, 2, 65) == 1  # 65 entries, one key, two groups of 64
    assert lib.ko_merge_worth(2 ** 32 - 1, 1, 2 ** 32 - 1) == 0  # the sum does not wrap


def test_run_region(lib):
    """lo[run_cap + 1] | slot[run_cap] | group_run0[G + 1], run_cap = distinct + G, in 32-bit words."""
    for distinct, G in ((1, 1), (1, 2), (3, 4), (175, 79), (0, 0)):
        out = np.zeros(5, np.uint64)
        lib.ko_region(distinct, G, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        cap = distinct + G
        assert [int(x) for x in out] == [cap, cap + 1, 2 * cap + 1, 2 * cap + 1 + G + 1, 4 * (2 * cap + 1 + G + 1)]


def test_key_order_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "keyorder"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "keyorder_san")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].endswith(" 0 wrong")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
