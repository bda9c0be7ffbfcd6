"""The canonical protobuf encoding of a tendermint.types.Block
(proto/tendermint/types/{block,types,evidence}.proto, version/types.proto) for
a host.FullBlock: what tmproto.Block.Marshal writes for it, with a map of
where every field sits, so that tests can mutate single fields.  Input
generation only: written from the proto3 encoding rules and gogoproto's
marshalling order (ascending field numbers, zero values omitted, the
nullable = false messages always written), never from the engine.

    Block      1 header, 2 data, 3 evidence, 4 last_commit (absent when nil)
    Header     1 version {1 block, 2 app}, 2 chain_id, 3 height, 4 time,
               5 last_block_id, 6..14 the hashes and the proposer address
    BlockID    1 hash, 2 part_set_header {1 total, 2 hash}
    Data       1 txs (repeated)
    EvidenceList 1 evidence (repeated; FullBlock.evidence holds each item's bytes)
    Commit     1 height, 2 round, 3 block_id, 4 signatures (repeated)
    CommitSig  1 block_id_flag, 2 validator_address, 3 timestamp {1 seconds, 2 nanos}, 4 signature
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Tuple

U64 = (1 << 64) - 1

# One encoded field.  path: dotted names from the block ("header.time.seconds",
# "last_commit.signatures[2].signature", "data.txs[0]").  tag: where its tag
# begins; at: where its varint value, or its length, begins; pos: where the
# payload begins (the varint itself for wire type 0); end: one past its last
# byte.  Positions count from the start of the block.
Field = namedtuple("Field", "path tag at pos end wire_type")

HASH_FIELDS = ("last_commit_hash", "data_hash", "validators_hash", "next_validators_hash", "consensus_hash",
               "app_hash", "last_results_hash", "evidence_hash", "proposer_address")


def uvarint(u: int) -> bytes:
    u &= U64
    out = bytearray()
    while u >= 0x80:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


class _Msg:
    def __init__(self):
        self.b = bytearray()
        self.fields: List[Field] = []

    def varint(self, num: int, v: int, path: str):
        """A proto3 scalar: absent when zero; negative int32 / int64 in the 10-byte form."""
        if v == 0:
            return
        tag = len(self.b)
        self.b += uvarint(num << 3)
        at = len(self.b)
        self.b += uvarint(v)
        self.fields.append(Field(path, tag, at, at, len(self.b), 0))

    def _delimited(self, num: int, payload: bytes, path: str) -> int:
        tag = len(self.b)
        self.b += uvarint(num << 3 | 2)
        at = len(self.b)
        self.b += uvarint(len(payload))
        pos = len(self.b)
        self.b += payload
        self.fields.append(Field(path, tag, at, pos, len(self.b), 2))
        return pos

    def bytes(self, num: int, data: bytes, path: str, repeated: bool = False):
        """bytes / string: absent when empty, unless an entry of a repeated field."""
        if data or repeated:
            self._delimited(num, data, path)

    def msg(self, num: int, sub: "_Msg", path: str):
        """An embedded message, written even when empty."""
        pos = self._delimited(num, bytes(sub.b), path)
        for f in sub.fields:
            self.fields.append(Field(path + "." + f.path, f.tag + pos, f.at + pos, f.pos + pos, f.end + pos,
                                     f.wire_type))


def _timestamp(t: Tuple[int, int]) -> _Msg:
    m = _Msg()
    m.varint(1, t[0], "seconds")
    m.varint(2, t[1], "nanos")
    return m


def _block_id(b) -> _Msg:
    psh = _Msg()
    psh.varint(1, b.psh_total, "total")
    psh.bytes(2, b.psh_hash, "hash")
    m = _Msg()
    m.bytes(1, b.hash, "hash")
    m.msg(2, psh, "part_set_header")
    return m


def _commit_sig(s) -> _Msg:
    m = _Msg()
    m.varint(1, s.block_id_flag, "block_id_flag")
    m.bytes(2, s.validator_address, "validator_address")
    m.msg(3, _timestamp(s.timestamp), "timestamp")
    m.bytes(4, s.signature, "signature")
    return m


def _commit(c) -> _Msg:
    m = _Msg()
    m.varint(1, c.height, "height")
    m.varint(2, c.round, "round")
    m.msg(3, _block_id(c.block_id), "block_id")
    for i, s in enumerate(c.signatures):
        m.msg(4, _commit_sig(s), "signatures[%d]" % i)
    return m


def _header(h, version: Optional[Tuple[int, int]]) -> _Msg:
    vb, va = version if version is not None else (h.version_block, h.version_app)
    v = _Msg()
    v.varint(1, vb, "block")
    v.varint(2, va, "app")
    m = _Msg()
    m.msg(1, v, "version")
    m.bytes(2, h.chain_id.encode(), "chain_id")
    m.varint(3, h.height, "height")
    m.msg(4, _timestamp(h.time), "time")
    m.msg(5, _block_id(h.last_block_id), "last_block_id")
    for k, name in enumerate(HASH_FIELDS):
        m.bytes(6 + k, getattr(h, name), name)
    return m


def encode_block(block, version: Optional[Tuple[int, int]] = None) -> Tuple[bytes, List[Field]]:
    """(the canonical bytes of a host.FullBlock, its field map).  version:
    (block, app) in place of the header's own."""
    data = _Msg()
    for i, t in enumerate(block.txs):
        data.bytes(1, t, "txs[%d]" % i, repeated=True)
    evidence = _Msg()
    for i, e in enumerate(block.evidence):
        evidence.bytes(1, e, "evidence[%d]" % i, repeated=True)
    m = _Msg()
    m.msg(1, _header(block.header, version), "header")
    m.msg(2, data, "data")
    m.msg(3, evidence, "evidence")
    if block.last_commit is not None:
        m.msg(4, _commit(block.last_commit), "last_commit")
    return bytes(m.b), m.fields


def field(fields: List[Field], path: str) -> Field:
    """The field map's entry for `path` (KeyError when the field is absent)."""
    for f in fields:
        if f.path == path:
            return f
    raise KeyError(path)
