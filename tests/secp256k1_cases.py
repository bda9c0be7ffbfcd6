"""Commit-level secp256k1 cases shared by the CPU suite (through the test
double, tests/test_secp256k1_commit.py) and the device suite
(tests/test_gpu_secp256k1.py).  Expected strings are the reference's:
  types/validation.go:313-315  "wrong signature (#%d): %X" of the signature
  crypto/ed25519/ed25519.go:214  "pubkey is not Ed25519" (BatchVerifier.Add)
"""
import hashlib
import random

import commit_fixtures as CF
from tendermint_amd import host as H
from tendermint_amd.testing import factory
from tendermint_amd.testing.secp256k1_factory import Secp256k1Signer

CHAIN = "secp-chain"


class SecpSigner:
    """A secp256k1 validator key (GenPrivKeySecp256k1 of "<tag>: <i>").  The
    address is supplied by the caller of the engine, never derived by it; the
    tests use SHA-256(pk)[:20] (the reference's RIPEMD160(SHA256(pk)) is not
    needed to check signatures)."""
    scheme = "secp256k1"

    def __init__(self, i: int, tag: str = "secp"):
        self._s = Secp256k1Signer.from_secret(f"{tag}: {i:x}".encode())
        self.pub_key = self._s.public_key
        self.kind = H.TMV_KIND_SECP256K1
        self.address = hashlib.sha256(self.pub_key).digest()[:20]

    def sign(self, msg: bytes) -> bytes:
        return self._s.sign(msg)


def val_set(signers, power=10, proposer_index=0):
    return H.ValidatorSet([H.Validator(s.address, s.pub_key, power, s.kind) for s in signers],
                          proposer_index=proposer_index)


def secp_set(n: int, power: int = 10):
    signers = sorted((SecpSigner(i) for i in range(n)), key=lambda s: s.address)
    return val_set(signers, power), signers


def mixed_set(n: int, ed_scheme: str, proposer_kind: int):
    """Alternating ed25519 (scheme "fake" for the CPU double, "ed25519" on the
    device) and secp256k1 validators; the proposer is the first of the kind."""
    signers = [SecpSigner(i, "mix") if i % 2 else CF.Signer(ed_scheme, i, "mix") for i in range(n)]
    signers.sort(key=lambda s: s.address)
    prop = next(i for i, s in enumerate(signers) if s.kind == proposer_kind)
    return val_set(signers, 10, prop), signers


def with_sig(commit: H.Commit, idx: int, sig: bytes) -> H.Commit:
    sigs = list(commit.signatures)
    c = sigs[idx]
    sigs[idx] = H.CommitSig(c.block_id_flag, c.validator_address, c.timestamp, sig)
    return H.Commit(commit.height, commit.round, commit.block_id, sigs)


def flip(sig: bytes) -> bytes:
    return bytes([sig[0] ^ 1]) + sig[1:]


def check_commit_cases(backend, n: int, ed_scheme: str):
    """The cases of the issue's test 2 over n validators through `backend`
    (verify_commit / verify_commit_light / verify_commit_light_trusting)."""
    assert n >= 6
    bid = CF.random_block_id(3)
    vals, signers = secp_set(n)
    commit = CF.make_commit(signers, CHAIN, 5, 0, bid)
    # a valid commit of an all-secp256k1 set
    assert backend.verify_commit(CHAIN, vals, bid, 5, commit) is None
    assert backend.verify_commit_light(CHAIN, vals, bid, 5, commit) is None
    assert backend.verify_commit_light_trusting(CHAIN, vals, commit) is None
    # a bad fourth signature: "wrong signature (#3): " + upper-case hex of the 64 bytes
    bad = flip(commit.signatures[3].signature)
    c_bad = with_sig(commit, 3, bad)
    want = "wrong signature (#3): " + bad.hex().upper()
    assert backend.verify_commit(CHAIN, vals, bid, 5, c_bad) == want
    assert backend.verify_commit_light(CHAIN, vals, bid, 5, c_bad) == want
    # trusting stops at > 1/3 (types/validation.go:96-132): signature #3 is reached only in larger sets
    k_third = (10 * n // 3) // 10 + 1  # signatures of power 10 needed to pass total / 3
    assert backend.verify_commit_light_trusting(CHAIN, vals, c_bad) == (want if k_third > 3 else None)
    # light returns nil once > 2/3 is tallied and ignores a later bad signature
    last = n - 1
    bad_last = flip(commit.signatures[last].signature)
    c_last = with_sig(commit, last, bad_last)
    assert backend.verify_commit_light(CHAIN, vals, bid, 5, c_last) is None
    assert backend.verify_commit(CHAIN, vals, bid, 5, c_last) == f"wrong signature (#{last}): " + bad_last.hex().upper()
    # an upper-S signature and a 63-byte signature are false
    s_int = int.from_bytes(commit.signatures[1].signature[32:], "big")
    from secp256k1_ref import N
    upper = commit.signatures[1].signature[:32] + (N - s_int).to_bytes(32, "big")
    assert backend.verify_commit(CHAIN, vals, bid, 5, with_sig(commit, 1, upper)) == \
        "wrong signature (#1): " + upper.hex().upper()
    short = commit.signatures[0].signature[:63]
    assert backend.verify_commit(CHAIN, vals, bid, 5, with_sig(commit, 0, short)) == \
        "wrong signature (#0): " + short.hex().upper()
    # a mixed set under a secp256k1 proposer: the single path, each entry by its own key type
    mvals, msigners = mixed_set(n, ed_scheme, H.TMV_KIND_SECP256K1)
    mcommit = CF.make_commit(msigners, CHAIN, 7, 0, bid)
    assert backend.verify_commit(CHAIN, mvals, bid, 7, mcommit) is None
    assert backend.verify_commit_light(CHAIN, mvals, bid, 7, mcommit) is None
    first = {k: next(i for i, s in enumerate(msigners) if s.kind == k)
             for k in (H.TMV_KIND_ED25519, H.TMV_KIND_SECP256K1)}
    for idx in sorted(first.values()):  # one of each key type
        b = flip(mcommit.signatures[idx].signature)
        assert backend.verify_commit(CHAIN, mvals, bid, 7, with_sig(mcommit, idx, b)) == \
            f"wrong signature (#{idx}): " + b.hex().upper()
    # the same set under an ed25519 proposer: the batch verifier's Add error
    evals, esigners = mixed_set(n, ed_scheme, H.TMV_KIND_ED25519)
    assert [s.pub_key for s in esigners] == [s.pub_key for s in msigners]
    assert backend.verify_commit(CHAIN, evals, bid, 7, mcommit) == "pubkey is not Ed25519"


def simple_validator_leaf(v) -> bytes:
    """SimpleValidator{pub_key: PublicKey{secp256k1 (field 2): pk}, voting_power}."""
    assert v.key_kind == H.TMV_KIND_SECP256K1 and v.voting_power < 128
    pub = bytes([0x12, len(v.pub_key)]) + v.pub_key
    return bytes([0x0A, len(pub)]) + pub + (bytes([0x10, v.voting_power]) if v.voting_power else b"")


def light_window(n_headers: int, n_vals: int):
    """(jobs, sets): sequential light verification of n_headers headers over
    one secp256k1 validator set, trusted header at height 1."""
    rng = random.Random(11)
    vals, signers = secp_set(n_vals)
    t0 = 1577836800
    shs, last = [], H.BlockID()
    for h in range(1, n_headers + 2):
        sh = factory._signed_header(H, CHAIN, h, 1, (t0 + h, 0), vals, vals, signers, last, rng)
        shs.append(sh)
        last = sh.commit.block_id
    jobs = [H.LightJob(shs[i], vals, shs[i + 1], vals, 3600 * 10**9, (t0 + n_headers + 10, 0))
            for i in range(n_headers)]
    return jobs, vals
