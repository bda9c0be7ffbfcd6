"""Split key scalars (tendermint_amd/csrc/split.h, compiled for the host into
tests/native/split with msm.h's parameters and recoding): relabelling the
digits of windows >= Ws onto the high point [2^(c Ws)]P leaves the scalar, the
digits and their number what they were, keeps every entry inside the windows a
split group sorts, and keeps a group inside its slots.  No GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libsplitcheck.so")
L_ORDER = 2**252 + 27742317777372353535851937790883648493
CS, MS = range(4, 10), range(5, 11)


@pytest.fixture(scope="module")
def C():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "split")], check=True)
    L = ctypes.CDLL(SO)
    u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    L.splitcheck_params.argtypes = [ctypes.c_uint32, ctypes.c_uint32, u32p]
    L.splitcheck_split_max.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.splitcheck_split_max.restype = ctypes.c_uint32
    L.splitcheck_entries.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, i32p, i32p, u32p, u32p]
    return L


def params(C, c, m_log2):
    out = np.zeros(9, np.uint32)
    assert C.splitcheck_params(c, m_log2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == 0
    return dict(zip(("W", "WR", "WL", "Ws", "Wa", "Wl", "cap", "H", "m"), (int(x) for x in out)))


def entries(C, s, c, m_log2, W):
    words = np.frombuffer(int(s).to_bytes(32, "little"), np.uint32).copy()
    lo, hi = np.zeros(W, np.int32), np.zeros(W, np.int32)
    unsplit, top = ctypes.c_uint32(), ctypes.c_uint32()
    n = C.splitcheck_entries(words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c, m_log2,
                             lo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                             hi.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(unsplit), ctypes.byref(top))
    return n, lo, hi, unsplit.value, top.value


def scalars(c, Ws, rng):
    edge = [0, 1, 2**(c * Ws) - 1, 2**(c * Ws), 2**(c * Ws) + 1, L_ORDER - 1, 2**252 - 1, 2**128 - 1, 2**128]
    edge += [sum((2**(c - 1)) << (c * w) for w in range(-(-252 // c))) % L_ORDER,       # every digit at the carry edge
             sum((2**(c - 1) - 1) << (c * w) for w in range(-(-252 // c))) % L_ORDER,   # ... just below it
             int("55" * 31, 16), int("0a" + "aa" * 31, 16)]
    return edge + [rng.randrange(L_ORDER) for _ in range(40)]


@pytest.mark.parametrize("c", CS)
def test_relabelled_digits_sum_to_the_scalar(C, c):
    rng = random.Random(c)
    for m_log2 in MS:
        p = params(C, c, m_log2)
        W, Ws = p["W"], p["Ws"]
        assert Ws == -(-W // 2) and p["Wa"] == max(Ws, p["WR"]) and p["Wl"] == max(Ws, p["WL"])
        for s in scalars(c, Ws, rng):
            n, lo, hi, unsplit, top = entries(C, s, c, m_log2, W)
            assert n >= 0, (c, m_log2, hex(s), n)
            low = sum(int(d) << (c * w) for w, d in enumerate(lo))
            high = sum(int(d) << (c * w) for w, d in enumerate(hi))
            assert low + (high << (c * Ws)) == s, (c, m_log2, hex(s))
            # the entry count is the unsplit recoding's
            assert n == unsplit == int(np.count_nonzero(lo)) + int(np.count_nonzero(hi))
            # every entry inside the windows a split group sorts (primary and located pass)
            assert top <= Ws <= p["Wa"] and top <= p["Wl"]
            assert not lo[Ws:].any() and not hi[Ws:].any()
            assert max(abs(int(d)) for d in list(lo) + list(hi)) <= p["H"]


@pytest.mark.parametrize("c", CS)
def test_group_stays_inside_its_slots(C, c):
    """cap bounds the entries of a group however its scalars are labelled
    (the digits do not change), and one window of a split group fits the
    2m + 1 entries k_msm_sort stages per window."""
    for m_log2 in MS:
        p = params(C, c, m_log2)
        m = p["m"]
        assert m * max(p["WR"], p["WL"]) + (m + 1) * p["W"] <= p["cap"]
        for want in (1, 4, 8, 16, 64, 10**6):
            smax = C.splitcheck_split_max(m, want)
            assert 1 <= smax <= want
            assert m + 2 * smax + 2 <= 2 * m + 1, (m, want, smax)


def test_sanitizer_program():
    """The same map as a stand-alone ASan + UBSan program."""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "split"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "split_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
