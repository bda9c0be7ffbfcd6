"""CPU restatement of what the block layer computes (TEST INFRASTRUCTURE: the
checker for tmv_commit_hashes, tmv_commit_hash_many, tmv_blocks_validate_basic
and chains.blocksync_replay_full; never imported by the product path).

Follows, in the reference:
  proto/tendermint/types/types.pb.go:1764-1797  CommitSig.MarshalToSizedBuffer
  types/block.go:900-918                        Commit.Hash
  types/block.go:53-94                          Block.ValidateBasic
  types/tx.go:34-39, types/evidence.go:667-678  Txs.Hash, EvidenceList.Hash
  types/part_set.go:172-222                     NewPartSetFromData(...).Header()
  internal/blocksync/reactor.go:563-586         the replay loop's checks per block pair
  internal/state/validation.go:14-96            validateBlock (the checks that need no application state)
hashlib, oracle/light_ref.py and oracle/merkle_ref.py only.  Works on the
host.* objects the product's Python layer takes.
"""
import hashlib

import chain_fixtures as CF
import light_ref as L
import merkle_ref as M

U64 = (1 << 64) - 1


def _uvarint(u: int) -> bytes:
    return M._varint(u & U64)


def _field(tag: int, b: bytes) -> bytes:
    return bytes([tag]) + _uvarint(len(b)) + b


def timestamp_bytes(secs: int, nanos: int) -> bytes:
    """google.protobuf.Timestamp{seconds, nanos}: zero fields omitted, negative
    values as 10-byte varints.  Equals light_ref.proto_timestamp inside the
    reference's domain (nanos in [0, 1e9))."""
    return (b"\x08" + _uvarint(secs) if secs else b"") + (b"\x10" + _uvarint(nanos) if nanos else b"")


def commit_sig_bytes(flag: int, addr: bytes, secs: int, nanos: int, sig: bytes) -> bytes:
    """tmproto.CommitSig{block_id_flag, validator_address, timestamp, signature}.Marshal()."""
    return ((b"\x08" + _uvarint(flag) if flag else b"") + (_field(0x12, addr) if addr else b"") +
            _field(0x1A, timestamp_bytes(secs, nanos)) + (_field(0x22, sig) if sig else b""))


def sig_bytes(s) -> bytes:
    """The bytes of a host.CommitSig."""
    return commit_sig_bytes(s.block_id_flag, s.validator_address, s.timestamp[0], s.timestamp[1], s.signature)


def commit_hash_of_sigs(sigs) -> bytes:
    """sigs: [(flag, addr, secs, nanos, sig)]."""
    return M.hash_from_byte_slices([commit_sig_bytes(*s) for s in sigs])


def commit_hash(c):
    """Commit.Hash of a host.Commit (None for a nil commit)."""
    return None if c is None else M.hash_from_byte_slices([sig_bytes(s) for s in c.signatures])


def txs_hash(txs) -> bytes:
    return M.hash_from_byte_slices([hashlib.sha256(t).digest() for t in txs])


def evidence_hash(evs) -> bytes:
    return M.hash_from_byte_slices(list(evs))


def part_set_header(raw: bytes, part_size: int):
    parts = [raw[i:i + part_size] for i in range(0, len(raw), part_size)]
    return len(parts), M.hash_from_byte_slices(parts)


def block_hash(b):
    """Block.Hash() of a block whose header is filled: Header.Hash()."""
    return L.header_hash(CF.header(b.header))


def block_validate_basic(b):
    """Block.ValidateBasic of a host.FullBlock: the error text or None.  The
    evidence items' own ValidateBasic is not part of the contract (they arrive
    encoded)."""
    h = b.header
    e = L.header_validate_basic(CF.header(h))
    if e:
        return "invalid header: " + e
    if b.last_commit is None:
        return "nil LastCommit"
    e = L.commit_validate_basic(CF.commit(b.last_commit))
    if e:
        return "wrong LastCommit: " + e
    for name, want, got in (("LastCommitHash", commit_hash(b.last_commit), h.last_commit_hash),
                            ("DataHash", txs_hash(b.txs), h.data_hash),
                            ("EvidenceHash", evidence_hash(b.evidence), h.evidence_hash)):
        if want != got:
            return "wrong Header.%s. Expected %s, got %s" % (name, L.hexu(want), L.hexu(got))
    return None


def _bid_str(b) -> str:
    return str(CF.block_id(b))


def replay_full(chain_id, vals, blocks, last_block_id, verify_light, verify_full, vals_hash, initial_height=1,
                part_size=65536, last_block_height=0):
    """The replay loop one block pair at a time.  verify_light / verify_full:
    (block_id, height, commit) -> error text or None (VerifyCommitLight /
    VerifyCommit over `vals`).  Returns (blocks applied, (height, error) or None)."""
    from tendermint_amd import host as H
    state_last, state_height = last_block_id, last_block_height
    for i in range(len(blocks) - 1):
        first, second = blocks[i], blocks[i + 1]
        total, phash = part_set_header(first.raw, part_size)
        first_id = H.BlockID(block_hash(first) or b"", total, phash)
        hd = first.header
        e = verify_light(first_id, hd.height, second.last_commit)
        if e is None:
            e = block_validate_basic(first)
        if e is None and hd.chain_id != chain_id:
            e = "wrong Block.Header.ChainID. Expected %s, got %s" % (chain_id, hd.chain_id)
        if e is None and state_height == 0 and hd.height != initial_height:
            e = "wrong Block.Header.Height. Expected %d for initial block, got %d" % (hd.height, initial_height)
        if e is None and state_height > 0 and hd.height != state_height + 1:
            e = "wrong Block.Header.Height. Expected %d, got %d" % (state_height + 1, hd.height)
        if e is None and not hd.last_block_id.equals(state_last):
            e = "wrong Block.Header.LastBlockID.  Expected %s, got %s" % (_bid_str(state_last),
                                                                        _bid_str(hd.last_block_id))
        if e is None and hd.validators_hash != vals_hash:
            e = "wrong Block.Header.ValidatorsHash.  Expected %s, got %s" % (L.hexu(vals_hash),
                                                                           L.hexu(hd.validators_hash))
        if e is None and hd.next_validators_hash != vals_hash:
            e = "wrong Block.Header.NextValidatorsHash.  Expected %s, got %s" % (L.hexu(vals_hash),
                                                                               L.hexu(hd.next_validators_hash))
        if e is None:
            if hd.height == initial_height:
                if first.last_commit.signatures:
                    e = "initial block can't have LastCommit signatures"
            else:
                e = verify_full(state_last, hd.height - 1, first.last_commit)
        if e is not None:
            return i, (hd.height, e)
        state_last, state_height = first_id, hd.height
    return len(blocks) - 1, None
