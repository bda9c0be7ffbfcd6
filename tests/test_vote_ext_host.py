"""Vote extensions on the host (no GPU): the C++ encoder of
VoteExtensionSignBytes against the checker (vote_ext_ref.py), the device's
length functions against the same, tmv_verify_extended_votes through the CPU
harness (tests/native/voteext: the product's host layer over an engine double
with the C oracle's signature checks), the extended VoteSet and
extended_commits_to_vote_sets."""
import ctypes
import os
import random
import re

import pytest

import vote_cases as V
import vote_ext_cases as X
import vote_ext_ref as R
from tendermint_amd import _native as N
from tendermint_amd import host as H
from tendermint_amd.types.canonical import vote_extension_sign_bytes
from tendermint_amd.vote_set import (VoteSet, extended_commit_ensure_extensions, extended_commit_validate_basic,
                                     vote_validate_basic)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_LENGTHS = [0, 1, 127, 128, 16383, 16384]


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "_build", "libvoteexthost.so"))
    lib.voteext_verify_extended_votes.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(H.CExtVoteIn),
                                                  ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32),
                                                  ctypes.POINTER(ctypes.c_uint8)]
    lib.voteext_device_msg_len.restype = ctypes.c_uint32
    lib.voteext_device_msg_len.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.voteext_device_wave_min.restype = ctypes.c_uint32
    lib.voteext_ripemd160.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return lib


@pytest.fixture(params=["host-built", "device-built"])
def backend(request, L, monkeypatch):
    """tmv_verify_extended_votes of the CPU harness, its messages built by
    the host encoder or sent as templates to the engine double."""
    monkeypatch.setenv("TMV_VOTE_EXT_DEVICE_MIN", "0" if request.param == "device-built" else "4000000000")
    fn = lambda h, *a: L.voteext_verify_extended_votes(*a)
    return lambda mode, chain, votes, keys: H.verify_extended_votes_call(fn, None, mode, chain, votes, keys)


@pytest.fixture(scope="module")
def sig_ok():
    return X.make_sig_ok()


@pytest.fixture(scope="module")
def mode_case(sig_ok):
    table = X.mode_table(X.table_vals())
    return table, {m: X.expected_mode_results(m, table, sig_ok) for m in (0, 1, 2)}


# ---------------------------------------------------------------- bytes
def test_known_vectors(L):
    """The two vectors derived by hand from the marshal code
    (proto/tendermint/types/canonical.pb.go:657-689)."""
    v1 = bytes.fromhex("230a09657874656e73696f6e110100000000000000220d746573745f636861696e5f6964")
    for f in (R.sign_bytes, vote_extension_sign_bytes, lambda *a: H.vote_extension_sign_bytes(*a, lib=L)):
        assert f("test_chain_id", 1, 0, b"extension") == v1 and len(v1) == 36
        assert f("", 0, 0, b"") == b"\x00"


def test_host_encoder_matches_checker(L):
    rng = random.Random(90)
    exts = {n: X.payload(rng, n) for n in EXT_LENGTHS}
    for c in V.CHAIN_IDS:
        for h in V.HEIGHTS:
            for r in V.ROUNDS:
                tail = H.vote_extension_template(c, h, r, lib=L)
                assert tail == R.tail(c, h, r)
                for n, e in exts.items():
                    want = R.sign_bytes(c, h, r, e)
                    assert H.vote_extension_sign_bytes(c, h, r, e, lib=L) == want
                    assert vote_extension_sign_bytes(c, h, r, e) == want
                    assert L.voteext_device_msg_len(len(tail), n) == len(want)  # the kernel's sizing


def test_length_prefix_boundaries(L):
    got = [R.ext_len_for_body(*X.BOUNDARY_TEMPLATE, b) for b in (127, 128, 16383, 16384)]
    assert got == X.BOUNDARY_LENGTHS == [92, 93, 16347, 16348]
    for e, total in zip(X.BOUNDARY_LENGTHS, (128, 130, 16385, 16387)):
        m = H.vote_extension_sign_bytes(*X.BOUNDARY_TEMPLATE, b"\x07" * e, lib=L)
        assert len(m) == total and m == R.sign_bytes(*X.BOUNDARY_TEMPLATE, b"\x07" * e)
        assert L.voteext_device_msg_len(len(R.tail(*X.BOUNDARY_TEMPLATE)), e) == total


def test_wave_copy_cutoff_constant(L):
    """The Python copy of kVoteExtWaveMin (the GPU tests straddle it)."""
    assert L.voteext_device_wave_min() == N.VOTE_EXT_WAVE_MIN
    with open(os.path.join(REPO, "tendermint_amd", "csrc", "vote_ext.h")) as f:
        assert int(re.search(r"kVoteExtWaveMin = (\d+);", f.read()).group(1)) == N.VOTE_EXT_WAVE_MIN


def test_ripemd160_vectors(L):
    for m, want in ((b"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"),
                    (b"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"),
                    (b"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"),
                    (b"a" * 1000000, "52783243c1697bdbe16d37f97f68f08325dc1528")):
        out = ctypes.create_string_buffer(20)
        L.voteext_ripemd160(m, len(m), out)
        assert out.raw.hex() == want
        if len(m) < 100:
            assert R.ripemd160(m).hex() == want


# ---------------------------------------------------------------- tmv_verify_extended_votes
def test_mode_table(backend, mode_case):
    X.check_mode_table(backend, *mode_case)


def test_vote_extension_cases_of_the_reference(backend):
    """TestVoteExtension (types/vote_test.go:227-290): VerifyExtension of a
    non-nil precommit with / without extension and extension signature."""
    val = X.Val(R.KIND_ED25519, 30)
    for ext, include_sig, expect_error in ((b"extension", True, False), (b"extension", False, True),
                                           (b"", True, False), (b"", False, True)):
        v = X.signed_vote(val, 0, ext=ext)
        if not include_sig:
            v.extension_signature = b""
        (res, failed), = backend(R.MODE_EXTENSION, X.CHAIN, [v], [val.key])
        assert (res, failed) == ((R.ERR_SIGNATURE, 2) if expect_error else (R.OK, 0))


# ---------------------------------------------------------------- VoteSet
def _vote_set(backend, n=7, enabled=True, msg_type=H.PRECOMMIT_TYPE):
    vals = sorted((X.Val(R.KIND_ED25519, 40 + i) for i in range(n)), key=lambda v: v.address)
    vset = H.ValidatorSet([H.Validator(v.address, v.pub_key, 1) for v in vals], proposer_index=0)
    plain = lambda c, v, k: [r for r, _ in backend(R.MODE_VERIFY, c, v, k)]
    return VoteSet(X.CHAIN, 1, 0, msg_type, vset, plain, enabled, X.vote_and_extension(backend)), vals


def test_extended_vote_set_rejects_forged_extension_signature(backend):
    """NewExtendedVoteSet's AddVote runs VerifyVoteAndExtension
    (types/vote_set.go:209-213): a precommit whose vote signature is good and
    whose extension signature is forged is ErrVoteInvalidSignature."""
    vs, vals = _vote_set(backend)
    assert vs.add_vote(X.signed_vote(vals[0], 0, ext=b"ext 0")) == (True, None)
    v = X.signed_vote(vals[1], 1, ext=b"ext 1")
    v.extension_signature = X._flip(v.extension_signature, 0)
    added, err = vs.add_vote(v)
    assert not added and err == ("failed to verify vote with ChainID %s and PubKey PubKeyEd25519{%s}: "
                                 "invalid signature" % (X.CHAIN, vals[1].pub_key.hex().upper()))
    assert vs.get_by_index(1) is None
    v = X.signed_vote(vals[2], 2, ext=b"ext 2")
    v.extension = b"ext 3"  # another extension than the one signed
    assert vs.add_vote(v)[1].endswith(": invalid signature")
    # a nil precommit's extension data is not looked at by the signature check
    v = X.signed_vote(vals[3], 3, bid=H.BlockID())
    v.extension_signature = b"\x01" * 64
    assert vs.add_vote(v) == (True, None)


def test_plain_vote_set_rejects_extension_data(backend):
    """types/vote_set.go:214-220."""
    vs, vals = _vote_set(backend, enabled=False)
    assert vs.add_vote(X.signed_vote(vals[0], 0, ext=b"e")) == (False, "unexpected vote extension data present in vote")
    v = X.signed_vote(vals[1], 1, bid=H.BlockID())
    assert vs.add_vote(v) == (True, None)
    v = X.signed_vote(vals[2], 2, ext=b"e")
    v.signature = X._flip(v.signature, 1)  # the signature check comes first
    assert vs.add_vote(v)[1].endswith(": invalid signature")


@pytest.mark.parametrize("seed", [1, 2])
def test_extended_batched_equals_sequential(backend, seed):
    rng = random.Random(seed)
    vs1, vals = _vote_set(backend, 9)
    vs2, _ = _vote_set(backend, 9)
    stream = []
    for _ in range(40):
        i = rng.randrange(9)
        v = X.signed_vote(vals[i], i, bid=rng.choice([H.BlockID(), X.BLOCK, X.BLOCK]), ext=b"e%d" % rng.randrange(3),
                          ts=(1600000000 + rng.randrange(3), 0))
        r = rng.random()
        if r < 0.1:
            v.signature = X._flip(v.signature, 5)
        elif r < 0.25 and v.extension_signature:
            v.extension_signature = X._flip(v.extension_signature, 9)
        elif r < 0.3:
            v.extension_signature = b""
        elif r < 0.35:
            v.validator_index = (i + 1) % 9
        stream.append(v)
    seq = [vs1.add_vote(v) for v in stream]
    assert vs2.add_votes(stream) == seq and vs2.signature_batches == 1
    assert [v and v.signature for v in vs1.votes] == [v and v.signature for v in vs2.votes]
    assert vs1.maj23 == vs2.maj23 and vs1.sum == vs2.sum
    assert sum(1 for a, _ in seq if a) >= 4 and sum(1 for _, e in seq if e and e.endswith("invalid signature")) >= 3


# ---------------------------------------------------------------- extended commits
def test_extended_commits_to_vote_sets(backend, sig_ok):
    X.check_extended_commits(backend, sig_ok)


def test_extended_commit_restatements():
    _, _, cases = X.extended_commit_cases()
    by = dict(cases)
    assert extended_commit_validate_basic(by["good"]) is None and extended_commit_ensure_extensions(by["good"]) is None
    assert extended_commit_ensure_extensions(by["missing extension signature"]) == "vote extension data is missing"
    ec = by["absent entry"]
    assert extended_commit_validate_basic(ec) is None and extended_commit_ensure_extensions(ec) is None
    ec.extended_signatures[3].extension = b"x"
    assert extended_commit_validate_basic(ec) == ("wrong ExtendedCommitSig #3: vote extension signature absent on "
                                                  "vote with extension")
    assert extended_commit_validate_basic(H.ExtendedCommit(3, 0, H.BlockID(), [])) == "commit cannot be for nil block"
    v = X.signed_vote(X.Val(R.KIND_ED25519, 1), 0, H.PREVOTE_TYPE, ext=b"e", sign_ext=False)
    assert vote_validate_basic(v) == "unexpected vote extension"
    v = X.signed_vote(X.Val(R.KIND_ED25519, 1), 0, ext=b"e")
    assert vote_validate_basic(v) is None and vote_validate_basic(v) == R.vote_validate_basic(X.as_dict(v))
    v.extension_signature = b""
    assert vote_validate_basic(v) == R.vote_validate_basic(X.as_dict(v)) == (
        "vote extension signature absent on vote with extension")


def test_vote_ext_under_asan_ubsan():
    """The stand-alone sanitizer program over the same host code (CPU only)."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "voteext"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "voteext_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
