"""A lenient proto3 decoder of tendermint.types.Block (TEST INFRASTRUCTURE: the
oracle for "what would the reference have decoded" in the tests of
tmv_blocks_validate_wire; never imported by the product path).

Written from the rules of the reference's generated Unmarshal code
(proto/tendermint/types/{block,types}.pb.go, version/types.pb.go) and
gogoproto's StdTimeUnmarshal, not from the product's strict scanner:
  * unknown fields are skipped (wire types 0, 1, 2 and 5);
  * fields may come in any order; an embedded message that occurs twice is
    merged into the first, the last scalar / bytes / string wins, repeated
    fields append; a timestamp that occurs twice is replaced;
  * a varint may be padded up to 10 bytes (an 11th is an error) and what lies
    beyond 64 bits is dropped; an int32 / uint32 / enum keeps its low 32 bits;
  * a known field with another wire type, field number 0, wire types 3, 4, 6, 7
    and a length past the enclosing message are errors;
  * a timestamp outside seconds [-62135596800, 253402300799] or nanos
    [0, 999999999] is an error (validateTimestamp).
decode_block returns a host.FullBlock (raw = the bytes), or raises DecodeError
where the reference's Unmarshal fails.  A block with evidence raises
HasEvidence: FullBlock.evidence holds re-marshalled items, which this decoder
does not produce (the strict scanner never handles such a block).
"""
from tendermint_amd import host as H

U64 = (1 << 64) - 1


class DecodeError(Exception):
    pass


class HasEvidence(Exception):
    pass


def _varint(b: bytes, p: int, end: int):
    v, shift = 0, 0
    while True:
        if shift >= 64:
            raise DecodeError("varint overflow")
        if p >= end:
            raise DecodeError("unexpected EOF")
        c = b[p]
        p += 1
        v = (v | (c & 0x7F) << shift) & U64
        if c < 0x80:
            return v, p
        shift += 7


def _i64(v: int) -> int:
    return v - (1 << 64) if v >> 63 else v


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _fields(b: bytes, lo: int, hi: int, wire_types: dict):
    """(field number, varint value or (payload lo, hi)) of every known field in
    b[lo:hi], in order; unknown fields skipped."""
    p = lo
    while p < hi:
        tag, p = _varint(b, p, hi)
        num, wt = _i32(tag >> 3), tag & 7
        if num <= 0:
            raise DecodeError("illegal tag")
        if wt in (3, 4, 6, 7):
            raise DecodeError("wire type %d" % wt)
        if num in wire_types and wire_types[num] != wt:
            raise DecodeError("wrong wire type for field %d" % num)
        if wt == 0:
            v, p = _varint(b, p, hi)
        elif wt == 2:
            n, p = _varint(b, p, hi)
            if n >> 31 or p + n > hi:
                raise DecodeError("length past the message")
            v, p = (p, p + n), p + n
        else:
            n = 8 if wt == 1 else 4
            if p + n > hi:
                raise DecodeError("unexpected EOF")
            v, p = None, p + n
        if num in wire_types:
            yield num, v


def _timestamp(b, lo, hi):
    secs = nanos = 0
    for num, v in _fields(b, lo, hi, {1: 0, 2: 0}):
        if num == 1:
            secs = _i64(v)
        else:
            nanos = _i32(v)
    if not (-62135596800 <= secs <= 253402300799 and 0 <= nanos <= 999999999):
        raise DecodeError("timestamp outside the domain")
    return secs, nanos


def _block_id(b, lo, hi, into: H.BlockID):
    for num, v in _fields(b, lo, hi, {1: 2, 2: 2}):
        if num == 1:
            into.hash = b[v[0]:v[1]]
        else:
            for n2, v2 in _fields(b, v[0], v[1], {1: 0, 2: 2}):
                if n2 == 1:
                    into.psh_total = v2 & 0xFFFFFFFF
                else:
                    into.psh_hash = b[v2[0]:v2[1]]


def _commit_sig(b, lo, hi) -> H.CommitSig:
    s = H.CommitSig(0, b"", (0, 0), b"")  # a zero tmproto.CommitSig: time.Time{} arrives as an explicit timestamp
    seen_time = False
    for num, v in _fields(b, lo, hi, {1: 0, 2: 2, 3: 2, 4: 2}):
        if num == 1:
            s.block_id_flag = _i32(v)
        elif num == 2:
            s.validator_address = b[v[0]:v[1]]
        elif num == 3:
            s.timestamp, seen_time = _timestamp(b, v[0], v[1]), True
        else:
            s.signature = b[v[0]:v[1]]
    if not seen_time:
        s.timestamp = H.ZERO_TIME  # the Go zero value of a non-nullable stdtime
    return s


def _commit(b, lo, hi, into: H.Commit):
    for num, v in _fields(b, lo, hi, {1: 0, 2: 0, 3: 2, 4: 2}):
        if num == 1:
            into.height = _i64(v)
        elif num == 2:
            into.round = _i32(v)
        elif num == 3:
            _block_id(b, v[0], v[1], into.block_id)
        else:
            into.signatures.append(_commit_sig(b, v[0], v[1]))


def _header(b, lo, hi, h: H.Header):
    names = {6 + k: f for k, f in enumerate(H._HASH_FIELDS)}
    wt = {1: 2, 2: 2, 3: 0, 4: 2, 5: 2}
    wt.update({k: 2 for k in names})
    for num, v in _fields(b, lo, hi, wt):
        if num == 1:
            for n2, v2 in _fields(b, v[0], v[1], {1: 0, 2: 0}):
                if n2 == 1:
                    h.version_block = v2
                else:
                    h.version_app = v2
        elif num == 2:
            h.chain_id = b[v[0]:v[1]].decode("latin-1")
        elif num == 3:
            h.height = _i64(v)
        elif num == 4:
            h.time = _timestamp(b, v[0], v[1])
        elif num == 5:
            _block_id(b, v[0], v[1], h.last_block_id)
        else:
            setattr(h, names[num], b[v[0]:v[1]])


def decode_block(b: bytes) -> H.FullBlock:
    hdr = H.Header("", 0, H.ZERO_TIME, H.BlockID(), version_block=0, version_app=0)
    blk = H.FullBlock(hdr, [], [], None, b)
    for num, v in _fields(b, 0, len(b), {1: 2, 2: 2, 3: 2, 4: 2}):
        if num == 1:
            _header(b, v[0], v[1], hdr)
        elif num == 2:
            for _, v2 in _fields(b, v[0], v[1], {1: 2}):
                blk.txs.append(b[v2[0]:v2[1]])
        elif num == 3:
            for _, v2 in _fields(b, v[0], v[1], {1: 2}):
                raise HasEvidence()
        else:
            if blk.last_commit is None:
                blk.last_commit = H.Commit(0, 0, H.BlockID(), [])
            _commit(b, v[0], v[1], blk.last_commit)
    return blk
