"""The column order of multi-batch launches (tendermint_amd/csrc/colorder.h,
compiled for the host into tests/native/colorder): the slot function is a
bijection onto [0, N) for ragged launches with empty batches, lays equal-size
batches out column by column inside tiles of T batches, and is the identity
for T = 0 and for one batch.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libcolordercheck.so")
KS = [1, 2, 63, 64, 65, 256]


@pytest.fixture(scope="module")
def C():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "colorder")], check=True)
    L = ctypes.CDLL(SO)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.colordercheck_permutation.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, u32p]
    L.colordercheck_permutation.restype = ctypes.c_int64
    L.colordercheck_slot.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.colordercheck_slot.restype = ctypes.c_int64
    return L


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def permutation(C, counts, T):
    counts = np.ascontiguousarray(counts, np.uint32)
    idx = np.zeros(max(int(counts.sum()), 1), np.uint32)
    bad = C.colordercheck_permutation(_u32(counts), len(counts), T, _u32(idx))
    return bad, idx[:int(counts.sum())]


def python_slot(counts, T, j, i):
    """The issue's formula, restated."""
    counts = [int(c) for c in counts]
    if T == 0 or len(counts) <= 1:
        return sum(counts[:j]) + i
    t0 = j // T * T
    tile = range(t0, min(t0 + T, len(counts)))
    return sum(counts[:t0]) + sum(min(counts[b], i) for b in tile) + sum(1 for b in tile if b < j and counts[b] > i)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", [1, 3, 64, 256])
def test_ragged_bijection(C, K, T):
    rng = np.random.default_rng(1000 * K + T)
    for _ in range(4):
        counts = rng.integers(0, 90, K).astype(np.uint32)
        counts[rng.random(K) < 0.25] = 0  # empty batches
        bad, idx = permutation(C, counts, T)
        assert bad == 0
        assert np.array_equal(np.sort(idx), np.arange(int(counts.sum()), dtype=np.uint32))
        # spot-check the device function against the formula
        for _ in range(20):
            j = int(rng.integers(0, K))
            if counts[j] == 0:
                continue
            i = int(rng.integers(0, counts[j]))
            assert C.colordercheck_slot(_u32(counts), K, T, j, i) == python_slot(counts, T, j, i)


@pytest.mark.parametrize("K", KS)
def test_equal_batches_are_columns(C, K):
    n, T = 37, 64
    counts = np.full(K, n, np.uint32)
    bad, idx = permutation(C, counts, T)
    assert bad == 0
    for t0 in range(0, K, T):
        rows = min(T, K - t0)
        tile = idx[t0 * n:(t0 + rows) * n].astype(np.int64).reshape(n, rows)
        # slots [c rows, (c + 1) rows) of the tile: entry c of batches t0 .. t0 + rows - 1
        want = (t0 + np.arange(rows))[None, :] * n + np.arange(n)[:, None]
        assert np.array_equal(tile, want)


@pytest.mark.parametrize("K", KS)
def test_tile_zero_and_one_batch_are_the_identity(C, K):
    rng = np.random.default_rng(K)
    counts = rng.integers(0, 50, K).astype(np.uint32)
    bad, idx = permutation(C, counts, 0)
    assert bad == 0 and np.array_equal(idx, np.arange(int(counts.sum()), dtype=np.uint32))
    bad, idx = permutation(C, counts[:1] + 1, 64)
    assert bad == 0 and np.array_equal(idx, np.arange(int(counts[0]) + 1, dtype=np.uint32))


def test_sanitizer_program():
    """The same checks as a stand-alone ASan + UBSan program."""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "colorder"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "colorder_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
