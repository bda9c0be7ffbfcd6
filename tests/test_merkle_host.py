"""The host fallback of tmv_part_set_headers, tmv_part_set_proofs,
tmv_parts_verify and tmv_proofs_verify: the host layer built without the
engine (tests/native/merkle, libmerklehost.so: its weak references to the
engine stay null) against the restatement of the reference.  No GPU."""
import ctypes
import os

import pytest

import merkle_host_cases as C
from tendermint_amd import host as H
from tendermint_amd._native import NativeError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libmerklehost.so")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return ctypes.CDLL(LIB)


@pytest.mark.parametrize("part_size", [C.PART, 4096])
def test_part_sets(lib, part_size):
    C.check_part_sets(None, lib, part_size)


def test_proofs_verify_texts(lib):
    C.check_proofs_verify(None, lib)


def test_argument_errors_and_empty_calls(lib):
    with pytest.raises(NativeError, match=r"\(-1\)"):
        H.part_set_headers(None, [b"abc"], 0, lib=lib)
    with pytest.raises(NativeError, match=r"\(-1\)"):
        H.part_set_proofs(None, [b"abc"], 0, lib=lib)
    assert H.part_set_headers(None, [], 4, lib=lib) == []
    assert H.part_set_proofs(None, [], 4, lib=lib) == []
    assert H.parts_verify(None, [], lib=lib) == []
    assert H.proofs_verify(None, [], lib=lib) == []
    # odd part sizes and a partial last part
    got = H.part_set_proofs(None, [b"0123456789"], 3, lib=lib)
    assert got[0][0] == 4 and [p.index for p in got[0][2]] == [0, 1, 2, 3]
