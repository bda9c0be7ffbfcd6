"""Writes tests/golden/light_wire_vectors.json: a few tiny light blocks whose
protobuf bytes are spelled out here by hand from the proto3 encoding rules
(tag = field << 3 | wire type, base-128 varints, length-delimited messages;
field numbers of proto/tendermint/types/{types,validator}.proto and
proto/tendermint/crypto/keys.proto), with entries of their field maps, their
hashes and what LightBlock.ValidateBasic says.  They pin
testing/light_wire.py's encoder and tests/light_wire_ref.py's decoder to bytes
that neither of them made.  The two hashes that a light block carries about
itself (the header's validators_hash, the commit's block id) are spliced into
the hand-written bytes from hashlib over hand-written leaves.

    python tests/golden/make_light_wire_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE),
                os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]

import merkle_ref as M  # noqa: E402
from tendermint_amd import host as H  # noqa: E402

CHAIN = "c"
ED, SR, SECP = 0, 1, 3  # TMV_KIND_*


def hx(*pieces) -> bytes:
    return bytes.fromhex("".join(pieces).replace(" ", ""))


# ---- four validators: (host.Validator, its Validator message, its SimpleValidator message)
# V1: ed25519, power 5, priority 0 (absent)
V1 = (H.Validator(b"\x11" * 20, b"\xa1" * 32, 5, ED, 0),
      hx("0a 14", "11" * 20, "12 22 0a 20", "a1" * 32, "18 05"),                      # 60 bytes
      hx("0a 22 0a 20", "a1" * 32, "10 05"))
# V2: secp256k1 (33 bytes, oneof field 2), power 0 (absent), priority -1 (the 10-byte varint)
V2 = (H.Validator(b"\x22" * 20, b"\x02" + b"\xb2" * 32, 0, SECP, -1),
      hx("0a 14", "22" * 20, "12 23 12 21 02", "b2" * 32, "20 ff ff ff ff ff ff ff ff ff 01"),  # 70 bytes
      hx("0a 23 12 21 02", "b2" * 32))
# V3: sr25519 (oneof field 3), power 300 (ac 02), priority 7
V3 = (H.Validator(b"\x33" * 20, b"\xc3" * 32, 300, SR, 7),
      hx("0a 14", "33" * 20, "12 22 1a 20", "c3" * 32, "18 ac 02 20 07"),             # 63 bytes
      hx("0a 22 1a 20", "c3" * 32, "10 ac 02"))
# V4: ed25519, power -2 (fe ff ff ff ff ff ff ff ff 01)
V4 = (H.Validator(b"\x44" * 20, b"\xd4" * 32, -2, ED, 0),
      hx("0a 14", "44" * 20, "12 22 0a 20", "d4" * 32, "18 fe ff ff ff ff ff ff ff ff 01"),  # 69 bytes
      hx("0a 22 0a 20", "d4" * 32, "10 fe ff ff ff ff ff ff ff ff 01"))


def header_bytes(vals_hash: bytes) -> bytes:
    return hx("0a 02 08 0b",               # version {block 11}
              "12 01 63",                  # chain_id "c"
              "18 01",                     # height 1
              "22 02 08 01",               # time {seconds 1}
              "2a 02 12 00",               # last_block_id {part_set_header {}}
              "42 20", vals_hash.hex(),    # validators_hash (field 8)
              "72 14", "55" * 20)          # proposer_address (field 14): 73 bytes


def header_hash(vals_hash: bytes) -> bytes:
    """Header.Hash (types/block.go:447-478): the 14 leaves, absent fields empty."""
    leaves = [hx("08 0b"), hx("0a 01 63"), hx("08 01"), hx("08 01"), hx("12 00"), b"", b"",
              hx("0a 20") + vals_hash, b"", b"", b"", b"", b"", hx("0a 14", "55" * 20)]
    return M.hash_from_byte_slices(leaves)


def commit_bytes(block_hash: bytes) -> bytes:
    return hx("08 01",                                                   # height 1
              "1a 48 0a 20", block_hash.hex(), "12 24 08 01 12 20", "77" * 32,   # block_id
              "22 5e 08 02 12 14", "11" * 20, "1a 02 08 01 22 40", "66" * 64)   # one signature: 172 bytes


def light_block(vals, proposer, total_hex, commit=True):
    """(host.LightBlock, bytes, header hash, validator set hash)."""
    vh = M.hash_from_byte_slices([v[2] for v in vals])
    hh = header_hash(vh)
    bid = H.BlockID(hh, 1, b"\x77" * 32)
    hdr = H.Header(CHAIN, 1, (1, 0), validators_hash=vh, proposer_address=b"\x55" * 20)
    c = H.Commit(1, 0, bid, [H.CommitSig(2, b"\x11" * 20, (1, 0), b"\x66" * 64)]) if commit else None
    sh = hx("0a 49") + header_bytes(vh) + (hx("12 ac 01") + commit_bytes(hh) if commit else b"")
    vs = b"".join(hx("0a %02x" % len(v[1])) + v[1] for v in vals) + hx("12 %02x" % len(proposer[1])) + proposer[1] + \
        hx(total_hex)
    assert len(sh) in (75, 250) and len(vs) < 16384

    def ln(n):  # a length of one or two varint bytes
        return bytes([n]) if n < 128 else bytes([n & 0x7F | 0x80, n >> 7])
    wire = hx("0a") + ln(len(sh)) + sh + hx("12") + ln(len(vs)) + vs
    lb = H.LightBlock(H.SignedHeader(hdr, c), H.ValidatorSet([v[0] for v in vals], vals.index(proposer)))
    return lb, wire, hh, vh


# A: one ed25519 validator, who is the proposer; total_voting_power 5.
A = light_block([V1], V1, "18 05")
A_FIELDS = {"signed_header": [0, 1, 3, 253], "signed_header.header": [3, 4, 5, 78],
            "signed_header.commit": [78, 79, 81, 253], "validator_set": [253, 254, 255, 381],
            "validator_set.validators[0]": [255, 256, 257, 317],
            "validator_set.validators[0].address": [257, 258, 259, 279],
            "validator_set.validators[0].pub_key": [279, 280, 281, 315],
            "validator_set.validators[0].pub_key.ed25519": [281, 282, 283, 315],
            "validator_set.validators[0].voting_power": [315, 316, 316, 317],
            "validator_set.proposer": [317, 318, 319, 379], "validator_set.total_voting_power": [379, 380, 380, 381]}
# B: all three key types; the secp256k1 validator has power 0; the sr25519 one proposes; total 305 (b1 02).
B = light_block([V1, V2, V3], V3, "18 b1 02")
B_FIELDS = {"validator_set": [253, 254, 256, 523], "validator_set.validators[1]": [318, 319, 320, 390],
            "validator_set.validators[1].pub_key.secp256k1": [344, 345, 346, 379],
            "validator_set.validators[1].proposer_priority": [379, 380, 380, 390],
            "validator_set.validators[2].pub_key.sr25519": [416, 417, 418, 450],
            "validator_set.validators[2].voting_power": [450, 451, 451, 453],
            "validator_set.proposer": [455, 456, 457, 520], "validator_set.total_voting_power": [520, 521, 521, 523]}
# C: a power of 0 next to a negative power in the 10-byte form; the total a Go
# node would have cached is -2.  ValidatorSet.ValidateBasic refuses validator #1.
C = light_block([V2, V4], V2, "18 fe ff ff ff ff ff ff ff ff 01")
C_FIELDS = {"validator_set.validators[1].voting_power": [388, 389, 389, 399],
            "validator_set.total_voting_power": [471, 472, 472, 482]}
# D: a nil commit (SignedHeader.commit absent): SignedHeader.ValidateBasic says so.
D = light_block([V1], V1, "18 05", commit=False)
D_FIELDS = {"signed_header": [0, 1, 2, 77], "validator_set": [77, 78, 79, 205]}

ERRORS = {"ed25519": "", "mixed": "",
          "negative_power": "invalid validator set: invalid validator #1: validator has negative voting power",
          "nil_commit": "invalid signed header: missing commit"}


def describe(lb):
    def bid(x):
        return {"hash": x.hash.hex(), "psh_total": x.psh_total, "psh_hash": x.psh_hash.hex()}
    h, c = lb.signed_header.header, lb.signed_header.commit
    d = {"chain": h.chain_id, "height": h.height, "time": list(h.time), "last_block_id": bid(h.last_block_id),
         "version": [h.version_block, h.version_app]}
    d.update({f: getattr(h, f).hex() for f in H._HASH_FIELDS})
    return {"header": d,
            "commit": None if c is None else {
                "height": c.height, "round": c.round, "block_id": bid(c.block_id),
                "signatures": [{"flag": s.block_id_flag, "address": s.validator_address.hex(),
                                "timestamp": list(s.timestamp), "signature": s.signature.hex()}
                               for s in c.signatures]},
            "validators": [{"address": v.address.hex(), "pub_key": v.pub_key.hex(), "key_kind": v.key_kind,
                            "voting_power": v.voting_power, "proposer_priority": v.proposer_priority}
                           for v in lb.vals.validators],
            "proposer_index": lb.vals.proposer_index}


def main():
    out = []
    for name, (lb, wire, hh, vh), fields, total in (("ed25519", A, A_FIELDS, 5), ("mixed", B, B_FIELDS, 305),
                                                    ("negative_power", C, C_FIELDS, -2), ("nil_commit", D, D_FIELDS, 5)):
        out.append({"name": name, "chain_id": CHAIN, "light_block": describe(lb), "total_voting_power": total,
                    "wire": wire.hex(), "fields": fields, "header_hash": hh.hex(), "vals_hash": vh.hex(),
                    "error": ERRORS[name]})
    assert hashlib.sha256(b"").digest() == M.empty_hash()
    with open(os.path.join(HERE, "light_wire_vectors.json"), "w") as f:
        json.dump({"field_entry": ["tag", "at", "pos", "end"], "vectors": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
