"""Commit.Hash, Block.ValidateBasic and blocksync_replay_full on the CPU: the
host layer built without the engine (tests/native/blocks, libblockshost.so:
its weak references to the engine stay null) against the restatement of the
reference (tests/commit_hash_ref.py).  The GPU twin is tests/test_gpu_blocks.py."""
import ctypes
import os
import subprocess

import pytest

import blocks_cases as C
import commit_hash_ref as R
import merkle_ref as M
from tendermint_amd import chains, host as H
from tendermint_amd.testing.blocks import make_full_chain

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libblockshost.so")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    L.bk_commit_sig_encode.restype = ctypes.c_size_t
    L.bk_commit_sig_encode.argtypes = [ctypes.POINTER(H.CCommitSig), ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t]
    return L


def _encode(lib, flag, addr, secs, nanos, sig) -> bytes:
    k = H._Keep()
    c = H._c_commit(k, H.Commit(1, 0, H.BlockID(), [H.CommitSig(flag, addr, (secs, nanos), sig)]))
    out = (ctypes.c_uint8 * 512)()
    n = lib.bk_commit_sig_encode(c.sigs, out, 512)
    return bytes(out[:n])


def test_case_lengths():
    C.check_case_lengths()


@pytest.mark.parametrize("name", sorted(C.ENCODER_CASES))
def test_encoder_bytes(lib, name):
    case = C.ENCODER_CASES[name]
    assert _encode(lib, *case) == R.commit_sig_bytes(*case)


@pytest.mark.parametrize("name", sorted(C.OUT_OF_DOMAIN_CASES))
def test_encoder_bytes_outside_the_references_domain(lib, name):
    case = C.OUT_OF_DOMAIN_CASES[name]
    assert _encode(lib, *case) == R.commit_sig_bytes(*case)


def test_encoder_bytes_outside_the_engines_columns(lib):
    """What the engine refuses is the host encoder's: two-byte flags, odd
    address lengths, long signatures."""
    for case in [(128, C.ADDR, C.T, 1, C.SIG), (255, C.ADDR[:19], C.T, 1, C.SIG + b"\1"), (2, C.ADDR * 7, 0, 0, C.SIG * 3)]:
        assert _encode(lib, *case) == R.commit_sig_bytes(*case)


def test_commit_hashes_host(lib):
    import random
    rng = random.Random(3)
    commits = [[C.random_sig(rng) for _ in range(n)] for n in (0, 1, 2, 3, 7, 64, 65, 129)]
    commits.append(list(C.ENCODER_CASES.values()))
    commits.append([(200, C.ADDR[:19], 5, 5, C.SIG + b"\2")])
    hc = [C.host_commit(c) for c in commits]
    got = H.commit_hashes(None, hc[:4] + [None] + hc[4:], lib)
    want = [R.commit_hash_of_sigs(c) for c in commits]
    assert got == want[:4] + [None] + want[4:]
    assert got[0] == M.empty_hash()
    assert H.commit_hashes(None, [], lib) == []


def test_validate_basic_texts(lib):
    C.check_validate_basic(None, lib, C.window_blocks())


def test_validate_basic_argument_errors_and_empty(lib):
    assert H.blocks_validate_basic(None, [], lib) == []
    assert lib.tmv_blocks_validate_basic(None, None, 1, None, None, 0, None, None) < 0
    assert lib.tmv_commit_hash_many(None, None, 1, None, None) < 0


@pytest.fixture(scope="module")
def chain():
    vals, blocks, ids = make_full_chain(12, 4, C.CHAIN, seed=41, raw_len=(1, 300), part_size=128, txs=(1, 4))
    return vals, blocks, ids, C.SigCache()


@pytest.fixture(scope="module")
def fake():
    import commit_fixtures as F
    fb = F.FakeBackend()
    fb.real_signatures(True)
    yield fb
    fb.real_signatures(False)


@pytest.mark.parametrize("window,depth", [(1, 1), (5, 2), (100, 1)])
def test_blocksync_replay_full(lib, fake, chain, window, depth):
    import commit_fixtures as F
    vals, blocks, ids, cache = chain
    vh = M.validator_set_hash([(v.pub_key, v.key_kind, v.voting_power) for v in vals.validators])

    def run(bl, last, height):
        return chains.blocksync_replay_full(None, C.CHAIN, vals, bl, last, window=window, depth=depth, part_size=128,
                                            verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs), lib=lib,
                                            vals_hash=vh, last_block_height=height)
    C.check_replay(run, cache, vals, blocks, ids, 7, part_size=128)


def test_replay_needs_raw(lib, chain):
    import dataclasses
    vals, blocks, ids, _ = chain
    bl = [dataclasses.replace(blocks[0], raw=None)] + blocks[1:]
    with pytest.raises(ValueError, match="no raw bytes"):
        chains.blocksync_replay_full(None, C.CHAIN, vals, bl, H.BlockID(), verify_commits=lambda jobs: [], lib=lib,
                                     vals_hash=b"")


def test_blocks_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "blocks"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "blocks_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
