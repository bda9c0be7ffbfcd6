"""Checker for vote extensions: a restatement of the reference's marshal code
and checks that shares nothing with the product's Python.

  * sign_bytes            VoteExtensionSignBytes (types/vote.go:159-172) over
                          CanonicalVoteExtension.MarshalToSizedBuffer
                          (proto/tendermint/types/canonical.pb.go:657-689)
  * check_vote            Vote.Verify, VerifyVoteAndExtension, VerifyExtension
                          (types/vote.go:226-276)
  * vote_validate_basic   Vote.ValidateBasic (types/vote.go:281-345)
  * to_extended_vote_set  ExtendedCommit.ToExtendedVoteSet, vote by vote, with
                          votesFromExtendedCommit's panic texts
                          (types/block.go:1037-1071, internal/consensus/state.go:704-732)
  * ripemd160             for the address of a secp256k1 key

Signature verdicts come from `sig_ok(kind, pub_key, msg, sig) -> bool`, which
the tests build over oracle_c.  The reference holds no known-answer vector
for the extension sign-bytes (privval/file_test.go:303-335 compares two
calls), so these bytes are pinned by the marshal code alone.
"""
from __future__ import annotations

import hashlib
import struct

PREVOTE, PRECOMMIT = 1, 2
OK, ERR_ADDRESS, ERR_SIGNATURE = 0, 1, 2
MODE_VERIFY, MODE_VERIFY_AND_EXTENSION, MODE_EXTENSION = 0, 1, 2
KIND_ED25519, KIND_SR25519, KIND_SECP256K1 = 0, 1, 3
MAX_SIGNATURE_SIZE = 64  # types/vote.go: max(ed25519.SignatureSize, 64)


def _sov(v: int) -> bytes:  # encodeVarintCanonical
    out = bytearray()
    while v >= 1 << 7:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def marshal_canonical_vote_extension(extension: bytes, height: int, round_: int, chain_id: bytes) -> bytes:
    """MarshalToSizedBuffer writes back to front: chain_id (0x22), round (0x19),
    height (0x11), extension (0x0a); the buffer read front to back is the
    reverse."""
    parts = []
    if len(chain_id) > 0:
        parts.append(b"\x22" + _sov(len(chain_id)) + chain_id)
    if round_ != 0:
        parts.append(b"\x19" + struct.pack("<Q", round_ & (2**64 - 1)))
    if height != 0:
        parts.append(b"\x11" + struct.pack("<Q", height & (2**64 - 1)))
    if len(extension) > 0:
        parts.append(b"\x0a" + _sov(len(extension)) + extension)
    return b"".join(reversed(parts))


def sign_bytes(chain_id: str, height: int, round_: int, extension: bytes) -> bytes:
    bz = marshal_canonical_vote_extension(extension, height, round_, chain_id.encode())
    return _sov(len(bz)) + bz  # protoio.MarshalDelimited


def tail(chain_id: str, height: int, round_: int) -> bytes:
    """What the extension messages of one (chain_id, height, round) share."""
    return marshal_canonical_vote_extension(b"", height, round_, chain_id.encode())


def concat(msgs):
    """(concatenation, offsets) of a list of messages."""
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    return b"".join(msgs), off


def ext_len_for_body(chain_id: str, height: int, round_: int, body_len: int) -> int:
    """The extension length E at which len(body) == body_len (E > 0)."""
    t = len(tail(chain_id, height, round_))
    for k in range(1, 6):
        e = body_len - t - 1 - k
        if e > 0 and len(_sov(e)) == k:
            return e
    raise ValueError("no such length")


def block_id_is_nil(block_id) -> bool:
    """block_id = None or (hash, parts total, parts hash)."""
    return block_id is None or (len(block_id[0]) == 0 and block_id[1] == 0 and len(block_id[2]) == 0)


def check_vote(mode: int, chain_id: str, v: dict, kind: int, pub_key: bytes, sig_ok, vote_msg: bytes,
               addr=None):
    """(TMV_VOTE_* result, failed signature: 0 none, 1 vote, 2 extension) of one
    vote in the reference's order.  v: type, height, round, block_id,
    validator_address, signature, extension, extension_signature; vote_msg =
    VoteSignBytes of the vote (the tests take it from the sign-bytes mirror
    pinned by the reference's vectors)."""
    non_nil_precommit = v["type"] == PRECOMMIT and not block_id_is_nil(v["block_id"])
    if mode != MODE_EXTENSION:
        if (addr if addr is not None else key_address(kind, pub_key)) != v["validator_address"]:
            return ERR_ADDRESS, 0
        if not sig_ok(kind, pub_key, vote_msg, v["signature"]):
            return ERR_SIGNATURE, 1
    if mode != MODE_VERIFY and non_nil_precommit:
        m = sign_bytes(chain_id, v["height"], v["round"], v["extension"])
        if not sig_ok(kind, pub_key, m, v["extension_signature"]):
            return ERR_SIGNATURE, 2
    return OK, 0


# ---------------------------------------------------------------- RIPEMD-160 (secp256k1 addresses)
_RL = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8,
       3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12, 1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2,
       4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13]
_RR = [5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12, 6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2,
       15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13, 8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14,
       12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11]
_SL = [11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8, 7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12,
       11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5, 11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12,
       9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6]
_SR = [8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6, 9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11,
       9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5, 15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8,
       8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11]
_KL = [0x00000000, 0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xA953FD4E]
_KR = [0x50A28BE6, 0x5C4DD124, 0x6D703EF3, 0x7A6D76E9, 0x00000000]
_M32 = 0xFFFFFFFF


def _rol(x, s):
    return ((x << s) | (x >> (32 - s))) & _M32


def _f(j, x, y, z):
    r = j >> 4
    if r == 0:
        return x ^ y ^ z
    if r == 1:
        return (x & y) | (~x & _M32 & z)
    if r == 2:
        return (x | (~y & _M32)) ^ z
    if r == 3:
        return (x & z) | (y & ~z & _M32)
    return x ^ (y | (~z & _M32))


def ripemd160(m: bytes) -> bytes:
    """RIPEMD-160; test vectors of the paper in test_vote_ext_host.py."""
    h = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    m = m + b"\x80" + b"\0" * ((55 - len(m)) % 64) + struct.pack("<Q", 8 * len(m))
    for at in range(0, len(m), 64):
        x = struct.unpack("<16I", m[at:at + 64])
        a1, b1, c1, d1, e1 = h
        a2, b2, c2, d2, e2 = h
        for j in range(80):
            t = (_rol((a1 + _f(j, b1, c1, d1) + x[_RL[j]] + _KL[j >> 4]) & _M32, _SL[j]) + e1) & _M32
            a1, e1, d1, c1, b1 = e1, d1, _rol(c1, 10), b1, t
            t = (_rol((a2 + _f(79 - j, b2, c2, d2) + x[_RR[j]] + _KR[j >> 4]) & _M32, _SR[j]) + e2) & _M32
            a2, e2, d2, c2, b2 = e2, d2, _rol(c2, 10), b2, t
        t = (h[1] + c1 + d2) & _M32
        h = [t, (h[2] + d1 + e2) & _M32, (h[3] + e1 + a2) & _M32, (h[4] + a1 + b2) & _M32, (h[0] + b1 + c2) & _M32]
    return struct.pack("<5I", *h)


def key_address(kind: int, pub_key: bytes) -> bytes:
    """PubKey.Address(): SHA-256(key)[:20] (crypto.AddressHash) for ed25519 and
    sr25519, RIPEMD160(SHA256(key)) for secp256k1 (crypto/secp256k1/secp256k1.go)."""
    d = hashlib.sha256(pub_key).digest()
    return ripemd160(d) if kind == KIND_SECP256K1 else d[:20]


# ---------------------------------------------------------------- ToExtendedVoteSet, one vote at a time
def _hexu(b: bytes) -> str:
    return b.hex().upper()


def _pubkey_string(kind: int, pk: bytes) -> str:
    return {KIND_ED25519: "PubKeyEd25519{%s}", KIND_SR25519: "PubKeySr25519{%s}",
            KIND_SECP256K1: "PubKeySecp256k1{%s}"}[kind] % _hexu(pk)


def vote_validate_basic(v: dict):
    """Vote.ValidateBasic (types/vote.go:281-345) of a vote rebuilt from an
    extended commit: the checks such a vote can fail."""
    if len(v["validator_address"]) != 20:
        return "expected ValidatorAddress size to be 20 bytes, got %d bytes" % len(v["validator_address"])
    if len(v["signature"]) == 0:
        return "signature is missing"
    if len(v["signature"]) > MAX_SIGNATURE_SIZE:
        return "signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
    if v["type"] != PRECOMMIT or block_id_is_nil(v["block_id"]):
        if len(v["extension"]) > 0:
            return "unexpected vote extension"
        if len(v["extension_signature"]) > 0:
            return "unexpected vote extension signature"
    else:
        if len(v["extension_signature"]) > MAX_SIGNATURE_SIZE:
            return "vote extension signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
        if len(v["extension_signature"]) == 0 and len(v["extension"]) != 0:
            return "vote extension signature absent on vote with extension"
    return None


def to_extended_vote_set(chain_id: str, vals, ec: dict, sig_ok, vote_msg_of):
    """ExtendedCommit.ToExtendedVoteSet + votesFromExtendedCommit, vote by vote.
    vals: [(kind, pub_key, address, power)]; ec: height, round, block_id,
    sigs = [dict(flag, validator_address, timestamp, signature, extension,
    extension_signature)]; vote_msg_of(vote dict) = its VoteSignBytes.  Every
    validator index occurs once, so AddVote's duplicate and conflict branches
    cannot be reached.  Returns (None, block key of the 2/3 majority, indices
    added) or (text of the panic / error, None, None)."""
    if ec["height"] == 0:
        return "Cannot make VoteSet for height == 0, doesn't make sense.", None, None
    total = sum(p for _, _, _, p in vals)
    by_block, maj, added = {}, None, []
    for idx, s in enumerate(ec["sigs"]):
        if s["flag"] == 1:
            continue
        v = dict(type=PRECOMMIT, height=ec["height"], round=ec["round"],
                 block_id=ec["block_id"] if s["flag"] == 2 else None, timestamp=s["timestamp"],
                 validator_address=s["validator_address"], signature=s["signature"], extension=s["extension"],
                 extension_signature=s["extension_signature"])
        bad = vote_validate_basic(v)
        if bad:
            return "failed to validate vote reconstructed from LastCommit: " + bad, None, None
        err = None
        if idx >= len(vals):
            err = "cannot find validator %d in valSet of size %d: invalid validator index" % (idx, len(vals))
        else:
            kind, pk, addr, power = vals[idx]
            if addr != v["validator_address"]:
                err = ("vote.ValidatorAddress (%s) does not match address (%s) for vote.ValidatorIndex (%d)\n"
                       "Ensure the genesis file is correct across all validators: invalid validator address" %
                       (_hexu(v["validator_address"]), _hexu(addr), idx))
            else:
                res, _ = check_vote(MODE_VERIFY_AND_EXTENSION, chain_id, v, kind, pk, sig_ok, vote_msg_of(v),
                                    addr=key_address(kind, pk))
                if res != OK:
                    err = "failed to verify vote with ChainID %s and PubKey %s: %s" % (
                        chain_id, _pubkey_string(kind, pk),
                        "invalid validator address" if res == ERR_ADDRESS else "invalid signature")
        if err:
            return "failed to reconstruct vote set from extended commit: " + err, None, None
        key = None if block_id_is_nil(v["block_id"]) else tuple(v["block_id"])
        by_block[key] = by_block.get(key, 0) + power
        added.append(idx)
        if maj is None and by_block[key] >= total * 2 // 3 + 1:
            maj = (key,)
    if maj is None:
        return "extended commit does not have +2/3 majority", None, None
    return None, maj[0], added
