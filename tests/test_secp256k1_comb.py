"""The comb tables of cached secp256k1 keys (tendermint_amd/csrc/secp256k1.h:
build_comb, comb_store_affine, verify_chain_comb) compiled for the host with
limb-bound assertions (tests/native/secpcomb/secpcomb.cpp), against the
big-integer restatement tests/secp256k1_ref.py.  No GPU."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import secp256k1_comb_cases as CC
import secp256k1_ref as R
from tendermint_amd.testing import secp256k1_factory as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libsecpcomb.so")
P, N = R.P, R.N
WINDOWS, DIGITS, ENTRY_WORDS = 64, 15, 16


@pytest.fixture(scope="module")
def S():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "secpcomb")], check=True)
    L = ctypes.CDLL(SO)
    assert L.secpcomb_words() == WINDOWS * DIGITS * ENTRY_WORDS
    return L


def u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def entry(tab, j, d):
    """Entry (window j, digit d) of a comb as an affine point of integers."""
    w = tab[ENTRY_WORDS * (DIGITS * j + d - 1):][:ENTRY_WORDS]
    val = lambda ws: sum(int(x) << (32 * k) for k, x in enumerate(ws))  # noqa: E731
    return (val(w[:8]), val(w[8:]))


def test_table_entries_vs_big_integers(S):
    """Every entry of windows 0, 1, 31 and 63 and 64 more seeded (window,
    digit) pairs per key equal d 16^j Q as integers; a lane's window (the
    device's build order, one inversion per window) gives the same words."""
    rng = random.Random(0xC0B)
    privs = [1, 2, 3, N - 1, N - 2] + [rng.randrange(1, N) for _ in range(8)]
    for d_priv in privs:
        q = R.mul(d_priv, R.G)
        pk = R.compress(q)
        tab = np.zeros(WINDOWS * DIGITS * ENTRY_WORDS, np.uint32)
        assert S.secpcomb_key(pk, u32p(tab)) == 1
        pairs = [(j, d) for j in (0, 1, 31, 63) for d in range(1, 16)]
        pairs += [(rng.randrange(64), rng.randrange(1, 16)) for _ in range(64)]
        for j, d in pairs:
            assert entry(tab, j, d) == R.mul(d_priv * d * 16**j, R.G), (hex(d_priv), j, d)
        win = np.zeros(DIGITS * ENTRY_WORDS, np.uint32)
        for j in (0, 1, 31, 63):
            assert S.secpcomb_window(pk, j, u32p(win)) == 1
            assert np.array_equal(win, tab[DIGITS * ENTRY_WORDS * j:][:DIGITS * ENTRY_WORDS]), (hex(d_priv), j)
    g = np.zeros_like(tab)
    S.secpcomb_g(u32p(g))
    one = np.zeros_like(tab)
    assert S.secpcomb_key(R.compress(R.G), u32p(one)) == 1
    assert np.array_equal(g, one)


def test_unparsable_keys_get_the_stand_in(S):
    rng = random.Random(5)
    tab = np.zeros(WINDOWS * DIGITS * ENTRY_WORDS, np.uint32)
    g = np.zeros_like(tab)
    S.secpcomb_g(u32p(g))
    gx = R.GX.to_bytes(32, "big")
    for pk in (b"\x00" + gx, b"\x04" + gx, b"\x02" + P.to_bytes(32, "big"),
               b"\x02" + F.non_residue_x(rng).to_bytes(32, "big")):
        assert R.parse_pubkey(pk) is None
        assert S.secpcomb_key(pk, u32p(tab)) == 0
        assert np.array_equal(tab, g)


def test_golden_vectors_through_the_comb_chain(S, golden):
    vectors = golden("secp256k1_vectors.json")
    names = " ".join(v["name"] for v in vectors)
    assert len(vectors) >= 400 and "infinity/" in names and "key/prefix" in names
    bad = []
    for v in vectors:
        pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        z = hashlib.sha256(msg).digest()
        got, plain = S.secpcomb_verify(pk, z, sig), S.secpcomb_verify_plain(pk, z, sig)
        if got != int(v["valid"]) or plain != int(v["valid"]):
            bad.append(v["name"])
    assert not bad, bad


def test_doubling_case_key_is_the_generator(S):
    cases = CC.key1_cases()
    assert [c for _, _, c in cases] == [True] * 4 + [False] * 4
    pk = R.compress(R.G)
    for msg, sig, coincide in cases:
        z = hashlib.sha256(msg).digest()
        assert R.verify(pk, msg, sig)
        assert S.secpcomb_verify(pk, z, sig) == 1, (msg, coincide)
        bad = sig[:40] + bytes([sig[40] ^ 4]) + sig[41:]
        assert S.secpcomb_verify(pk, z, bad) == int(R.verify(pk, msg, bad)) == 0, (msg, coincide)


def test_comb_code_under_asan_ubsan():
    """The stand-alone sanitizer program (its own main) over the golden
    vectors; nothing is loaded into this interpreter."""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "secpcomb"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "secpcomb_san"),
                        os.path.join(REPO, "tests", "golden", "secp256k1_vectors.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
