"""Writes tests/golden/block_wire_vectors.json: a few tiny blocks whose
protobuf bytes are spelled out here by hand from the proto3 encoding rules
(tag = field << 3 | wire type, base-128 varints, length-delimited messages;
field numbers of proto/tendermint/types/{block,types}.proto), with entries of
their field maps and their hashes.  They pin testing/block_wire.py's encoder
and tests/block_wire_ref.py's decoder to bytes that neither of them made.
The hashes come from tests/commit_hash_ref.py (hashlib).

    python tests/golden/make_block_wire_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE),
                os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]

import commit_hash_ref as R  # noqa: E402
from tendermint_amd import host as H  # noqa: E402

T = 1577836800  # varint 80 c2 af f0 05
PART_SIZE = 64


def hx(*pieces) -> bytes:
    return bytes.fromhex("".join(pieces).replace(" ", ""))


# A: the smallest block that passes the scanner.  A commit without signatures
# (height 0, round 0, a zero BlockID) is present: 22 04 { 1a 02 { 12 00 } }.
A = (H.FullBlock(H.Header("c", 1, (1, 0), validators_hash=b"\xaa" * 32), [], [], H.Commit(0, 0, H.BlockID(), [])),
     hx("0a 33",                     # header, 51 bytes
        "0a 02 08 0b",               #   version {block 11}
        "12 01 63",                  #   chain_id "c"
        "18 01",                     #   height 1
        "22 02 08 01",               #   time {seconds 1}
        "2a 02 12 00",               #   last_block_id {part_set_header {}}
        "42 20", "aa" * 32,          #   validators_hash (field 8)
        "12 00",                     # data {}
        "1a 00",                     # evidence {}
        "22 04 1a 02 12 00"),        # last_commit {block_id {part_set_header {}}}
     {"header": [0, 1, 2, 53], "header.version": [2, 3, 4, 6], "header.version.block": [4, 5, 5, 6],
      "header.chain_id": [6, 7, 8, 9], "header.height": [9, 10, 10, 11], "header.time": [11, 12, 13, 15],
      "header.time.seconds": [13, 14, 14, 15], "header.last_block_id": [15, 16, 17, 19],
      "header.last_block_id.part_set_header": [17, 18, 19, 19], "header.validators_hash": [19, 20, 21, 53],
      "data": [53, 54, 55, 55], "evidence": [55, 56, 57, 57], "last_commit": [57, 58, 59, 63],
      "last_commit.block_id": [59, 60, 61, 63], "last_commit.block_id.part_set_header": [61, 62, 63, 63]})

# B: a nil commit (field 4 absent), an app version, a two-byte height, nanos,
# an empty transaction (0a 00) and a two-byte one.
B = (H.FullBlock(H.Header("t-1", 300, (T, 5), validators_hash=b"\xbb" * 32, version_app=2), [b"", b"ab"], [], None),
     hx("0a 3e",                                # header, 62 bytes
        "0a 04 08 0b 10 02",                    #   version {block 11, app 2}
        "12 03 74 2d 31",                       #   chain_id "t-1"
        "18 ac 02",                             #   height 300
        "22 08 08 80 c2 af f0 05 10 05",        #   time {seconds T, nanos 5}
        "2a 02 12 00",
        "42 20", "bb" * 32,
        "12 06 0a 00 0a 02 61 62",              # data {txs "", "ab"}
        "1a 00"),
     {"header.version.app": [6, 7, 7, 8], "header.height": [13, 14, 14, 16], "header.time.nanos": [24, 25, 25, 26],
      "data": [64, 65, 66, 72], "data.txs[0]": [66, 67, 68, 68], "data.txs[1]": [68, 69, 70, 72],
      "evidence": [72, 73, 74, 74]})

# C: a full BlockID, a proposer address (field 14: tag 72), a commit with an
# absent signature (flag 1 and Go's zero time, seconds -62135596800 in the
# 10-byte form) and a signed one; lengths of two bytes (b7 01, c5 01).
BID = H.BlockID(b"\x11" * 32, 1, b"\x22" * 32)
BID_HEX = ("0a 20" + "11" * 32 + "12 24 08 01 12 20" + "22" * 32)  # 72 bytes
C = (H.FullBlock(H.Header("t-1", 2, (T, 0), BID, last_commit_hash=b"\x33" * 32, validators_hash=b"\xcc" * 32,
                          proposer_address=b"\x44" * 20), [b"\x00"], [],
                 H.Commit(1, 1, BID, [H.CommitSig(), H.CommitSig(2, b"\x55" * 20, (T, 5), b"\x66" * 64)])),
     hx("0a b7 01",                             # header, 183 bytes
        "0a 02 08 0b", "12 03 74 2d 31", "18 02",
        "22 06 08 80 c2 af f0 05",              #   time {seconds T}
        "2a 48", BID_HEX,                       #   last_block_id
        "32 20", "33" * 32,                     #   last_commit_hash (field 6)
        "42 20", "cc" * 32,
        "72 14", "44" * 20,                     #   proposer_address (field 14)
        "12 03 0a 01 00",                       # data {txs 00}
        "1a 00",
        "22 c5 01",                             # last_commit, 197 bytes
        "08 01 10 01",                          #   height 1, round 1
        "1a 48", BID_HEX,
        "22 0f 08 01 1a 0b 08 80 92 b8 c3 98 fe ff ff ff 01",   # absent: flag 1, the zero time
        "22 64 08 02 12 14", "55" * 20, "1a 08 08 80 c2 af f0 05 10 05", "22 40", "66" * 64),
     {"header": [0, 1, 3, 186], "header.last_block_id.part_set_header.total": [60, 61, 61, 62],
      "header.proposer_address": [164, 165, 166, 186], "last_commit": [193, 194, 196, 393],
      "last_commit.round": [198, 199, 199, 200], "last_commit.signatures[0]": [274, 275, 276, 291],
      "last_commit.signatures[0].timestamp.seconds": [280, 281, 281, 291],
      "last_commit.signatures[1].signature": [327, 328, 329, 393]})


def describe(b):
    def bid(x):
        return {"hash": x.hash.hex(), "psh_total": x.psh_total, "psh_hash": x.psh_hash.hex()}
    h = b.header
    d = {"chain_id": h.chain_id, "height": h.height, "time": list(h.time), "last_block_id": bid(h.last_block_id),
         "version": [h.version_block, h.version_app]}
    d.update({f: getattr(h, f).hex() for f in H._HASH_FIELDS})
    c = b.last_commit
    return {"header": d, "txs": [t.hex() for t in b.txs],
            "last_commit": None if c is None else {
                "height": c.height, "round": c.round, "block_id": bid(c.block_id),
                "signatures": [{"flag": s.block_id_flag, "address": s.validator_address.hex(),
                                "timestamp": list(s.timestamp), "signature": s.signature.hex()}
                               for s in c.signatures]}}


def main():
    out = []
    for name, (b, wire, fields) in (("minimal", A), ("nil_commit", B), ("commit", C)):
        total, phash = R.part_set_header(wire, PART_SIZE)
        ch = R.commit_hash(b.last_commit)
        out.append({"name": name, "block": describe(b), "wire": wire.hex(), "fields": fields,
                    "header_hash": R.block_hash(b).hex(), "commit_hash": None if ch is None else ch.hex(),
                    "data_hash": R.txs_hash(b.txs).hex(), "validate_basic": R.block_validate_basic(b),
                    "part_size": PART_SIZE, "part_set_header": [total, phash.hex()]})
    with open(os.path.join(HERE, "block_wire_vectors.json"), "w") as f:
        json.dump({"field_entry": ["tag", "at", "pos", "end"], "vectors": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
