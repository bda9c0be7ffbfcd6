"""csrc/host/merkle_plan.h (aunt offsets, arena layout, leaves per wave of the
merkle proof entry points) through tests/native/merkle, against the recursive
restatement (tests/merkle_proof_ref.py), and the same header under
ASan + UBSan as a stand-alone program.  No GPU; nothing sanitized is loaded
into this interpreter."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import merkle_proof_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libmerklecheck.so")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    L.mp_split_point.restype = ctypes.c_uint64
    L.mp_split_point.argtypes = [ctypes.c_uint64]
    L.mp_aunt_count.restype = ctypes.c_uint32
    L.mp_aunt_count.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.mp_aunt_offsets.argtypes = [u32p, ctypes.c_uint32, u32p]
    L.mp_arena_base.restype = ctypes.c_uint64
    L.mp_arena_base.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.mp_leaves_per_wave.restype = ctypes.c_uint32
    L.mp_leaves_per_wave.argtypes = [ctypes.c_uint32]
    return L


def _offsets(lib, sizes):
    tree_off = np.zeros(len(sizes) + 1, np.uint32)
    tree_off[1:] = np.cumsum(sizes)
    out = np.full(int(tree_off[-1]) + 1, 0xFFFFFFFF, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = lib.mp_aunt_offsets(tree_off.ctypes.data_as(u32p), len(sizes), out.ctypes.data_as(u32p))
    return rc, out


def test_aunt_offsets_equal_the_restatement_up_to_1030(lib):
    """Every (index, total) with total <= 1,030, all trees in one call."""
    sizes = list(range(0, 1031))
    rc, out = _offsets(lib, sizes)
    assert rc == 0 and out[0] == 0
    counts = np.diff(out.astype(np.int64))
    want = np.array([P.aunt_count(i, n) for n in sizes for i in range(n)], np.int64)
    assert np.array_equal(counts, want)
    for n in (1, 2, 3, 5, 1030):
        for i in range(n):
            assert lib.mp_aunt_count(i, n) == P.aunt_count(i, n)


def test_aunt_counts_at_powers_of_two_up_to_2_31(lib):
    for k in range(1, 32):
        for total in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            if total < 1:
                continue
            if total >= 2:
                assert lib.mp_split_point(total) == P.split_point(total)
            k2 = P.split_point(total) if total >= 2 else 0
            for index in sorted({0, 1, k2 - 1, k2, k2 + 1, total // 3, total - 2, total - 1}):
                if 0 <= index < total:
                    assert lib.mp_aunt_count(index, total) == P.aunt_count(index, total), (index, total)


def test_empty_trees_between_and_bad_offsets(lib):
    sizes = [0, 1, 0, 0, 2, 3, 0, 17, 0]
    rc, out = _offsets(lib, sizes)
    assert rc == 0
    want = [P.aunt_count(i, n) for n in sizes for i in range(n)]
    assert np.diff(out.astype(np.int64)).tolist() == want
    tree_off = np.array([0, 5, 3], np.uint32)
    o = np.zeros(6, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert lib.mp_aunt_offsets(tree_off.ctypes.data_as(u32p), 2, o.ctypes.data_as(u32p)) == -1


def test_arena_holds_every_level(lib):
    """Level k >= 1 of a tree of n leaves has ceil(n / 2^k) nodes; the levels of
    tree t start at mp_arena_base(tree_off[t], t) and end before the next tree's."""
    def upper(n):
        s = 0
        while n > 1:
            n = (n + 1) // 2
            s += n
        return s
    sizes = [0, 1, 2, 3, 5, 0, 127, 128, 129, 1000, 2 ** 20 + 1]
    off = 0
    for t, n in enumerate(sizes):
        assert lib.mp_arena_base(off, t) + upper(n) <= lib.mp_arena_base(off + n, t + 1)
        off += n


def test_leaves_per_wave_rule(lib):
    """The measured boundaries: 8 to 2,048 leaves, 16 to 4,096, 32 to 16,384, then 64."""
    want = {1: 8, 256: 8, 1600: 8, 2048: 8, 2049: 16, 4096: 16, 4097: 32, 5120: 32, 10752: 32, 16384: 32,
            16385: 64, 21504: 64, 10 ** 6: 64}
    assert {n: lib.mp_leaves_per_wave(n) for n in want} == want


def test_plan_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "merkle"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "merkle_san")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
