"""secp256k1 validators through the host layer on the CPU: the product's
tm_host_abi.cpp inside the test double (tests/native/commit_check.cpp), which
defines no secp256k1 engine entry, so the host build of secp256k1.h verifies
(same code as the device).  The double's ed25519 signatures are its fake
scheme; secp256k1 signatures are real.  No GPU."""
import ctypes

import pytest

import commit_fixtures as CF
import merkle_ref as M
import secp256k1_cases as SC
from tendermint_amd import host as H


@pytest.fixture(scope="module")
def fake():
    return CF.FakeBackend()


def test_valid_all_secp256k1_commit(fake):
    """Fails without the feature: `wrong signature (#0)` for a valid commit."""
    bid = CF.random_block_id(1)
    vals, signers = SC.secp_set(6)
    commit = CF.make_commit(signers, SC.CHAIN, 3, 0, bid)
    assert fake.verify_commit(SC.CHAIN, vals, bid, 3, commit) is None
    assert fake.verify_commit_light(SC.CHAIN, vals, bid, 3, commit) is None
    assert fake.verify_commit_light_trusting(SC.CHAIN, vals, commit) is None


def test_commit_cases(fake):
    SC.check_commit_cases(fake, 7, "fake")


def test_many_commits_one_call(fake):
    """tmv_verify_commits: secp256k1 entries of several plans in one backend call."""
    bid = CF.random_block_id(2)
    vals, signers = SC.secp_set(6)
    commits = [CF.make_commit(signers, SC.CHAIN, h, 0, bid) for h in (1, 2, 3)]
    bad = SC.flip(commits[1].signatures[2].signature)
    commits[1] = SC.with_sig(commits[1], 2, bad)
    jobs = [H.CommitJob(H.MODE_FULL, SC.CHAIN, vals, bid, c.height, c) for c in commits]
    assert CF.fake_verify_commits(fake, jobs) == [None, "wrong signature (#2): " + bad.hex().upper(), None]


def test_validator_set_hash_matches_oracle(fake):
    """ValidatorSet.Hash of a secp256k1 set (host-hashed: oneof tag 0x12, 33-byte
    keys) equals the oracle's tree over the same leaves: a light verification
    whose headers carry the oracle's hash passes light/verifier.go:266."""
    jobs, vals = SC.light_window(2, 5)
    want = M.hash_from_byte_slices([SC.simple_validator_leaf(v) for v in vals.validators])
    for jb in jobs:
        assert jb.untrusted.header.validators_hash == want
    assert fake.light_verify_many(jobs) == [(H.LIGHT_OK, None)] * 2
    # another supplied set is refused, and the text carries the engine's hash of that set
    vals2 = H.ValidatorSet([H.Validator(v.address, v.pub_key, 11, v.key_kind) for v in vals.validators], 0)
    want2 = M.hash_from_byte_slices([SC.simple_validator_leaf(v) for v in vals2.validators])
    jb = jobs[1]
    code, err = fake.light_verify_many([H.LightJob(jb.trusted, vals, jb.untrusted, vals2, jb.trusting_period_ns,
                                                   jb.now)])[0]
    assert code != H.LIGHT_OK
    assert f"expected new header validators ({want.hex().upper()}) to match those that were supplied " \
           f"({want2.hex().upper()})" in err


def test_no_batch_verifier_for_secp256k1(fake):
    fake.L.commitcheck_ctx.restype = ctypes.c_void_p
    ctx = fake.L.commitcheck_ctx()
    assert H.create_batch_verifier(ctx, H.TMV_KIND_SECP256K1, fake.L) is None
    assert not H.supports_batch_verifier(H.TMV_KIND_SECP256K1)
    # a foreign key keeps the Add error of the batch's own type
    v = H.create_batch_verifier(ctx, H.TMV_KIND_ED25519, fake.L)
    key = SC.SecpSigner(0)
    assert v.add(H.TMV_KIND_SECP256K1, key.pub_key, b"m", key.sign(b"m")) == "pubkey is not Ed25519"
    v = H.create_batch_verifier(ctx, H.TMV_KIND_SR25519, fake.L)
    assert v.add(H.TMV_KIND_SECP256K1, key.pub_key, b"m", key.sign(b"m")) == "sr25519: pubkey is not sr25519"
