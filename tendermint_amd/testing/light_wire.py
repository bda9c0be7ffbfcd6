"""The canonical protobuf encoding of a tendermint.types.LightBlock
(proto/tendermint/types/{types,validator}.proto, crypto/keys.proto) for a
host.LightBlock: what tmproto.LightBlock.Marshal writes for it, with a map of
where every field sits, so that tests can mutate single fields.  Input
generation only, written from the proto3 encoding rules and gogoproto's
marshalling order, never from the engine; header and commit are
testing/block_wire.py's.

    LightBlock    1 signed_header, 2 validator_set     (pointers: absent when None)
    SignedHeader  1 header, 2 commit                    (pointers: absent when None)
    ValidatorSet  1 validators (repeated), 2 proposer (pointer), 3 total_voting_power
    Validator     1 address, 2 pub_key (always written), 3 voting_power, 4 proposer_priority
    PublicKey     oneof: 1 ed25519 | 2 secp256k1 | 3 sr25519  (written even when empty)
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from .block_wire import Field, _Msg, _commit, _header, field, uvarint  # noqa: F401  (re-exported)

KEY_FIELD = {0: (1, "ed25519"), 3: (2, "secp256k1"), 1: (3, "sr25519")}  # by TMV_KIND_*
AUTO = "auto"


def _public_key(v) -> _Msg:
    m = _Msg()
    if v.key_kind in KEY_FIELD:  # another kind: the oneof stays unset (not what a Go node can write)
        num, name = KEY_FIELD[v.key_kind]
        m.bytes(num, v.pub_key, name, repeated=True)  # a oneof member is written even when empty
    return m


def _validator(v) -> _Msg:
    m = _Msg()
    m.bytes(1, v.address, "address")
    m.msg(2, _public_key(v), "pub_key")
    m.varint(3, v.voting_power, "voting_power")
    m.varint(4, v.proposer_priority, "proposer_priority")
    return m


def proposer_of(vals):
    """ValidatorSet.GetProposer on a set whose proposer is not stored: the
    validator at proposer_index, else the highest priority, ties to the
    smaller address (types/validator_set.go:322-344); None for an empty set."""
    if not vals.validators:
        return None
    if 0 <= vals.proposer_index < len(vals.validators):
        return vals.validators[vals.proposer_index]
    best = None
    for v in vals.validators:
        if best is None or v.proposer_priority > best.proposer_priority or (
                v.proposer_priority == best.proposer_priority and v.address < best.address):
            best = v
    return best


def _validator_set(vals, proposer, total: Optional[int]) -> _Msg:
    m = _Msg()
    for i, v in enumerate(vals.validators):
        m.msg(1, _validator(v), "validators[%d]" % i)
    if proposer == AUTO:
        proposer = proposer_of(vals)
    if proposer is not None:
        m.msg(2, _validator(proposer), "proposer")
    m.varint(3, sum(v.voting_power for v in vals.validators) if total is None else total, "total_voting_power")
    return m


def encode_light_block(lb, proposer=AUTO, total: Optional[int] = None,
                       version: Optional[Tuple[int, int]] = None) -> Tuple[bytes, List[Field]]:
    """(the canonical bytes of a host.LightBlock, its field map).  A
    signed_header, header, commit or vals that is None is a nil pointer and is
    not written.  proposer: a host.Validator, None for a nil proposer, or AUTO
    for the set's own (proposer_of).  total: total_voting_power as the sender
    cached it (None: the sum; 0: not written).  version: (block, app) in place
    of the header's own."""
    m = _Msg()
    sh = lb.signed_header
    if sh is not None:
        s = _Msg()
        if sh.header is not None:
            s.msg(1, _header(sh.header, version), "header")
        if sh.commit is not None:
            s.msg(2, _commit(sh.commit), "commit")
        m.msg(1, s, "signed_header")
    if lb.vals is not None:
        m.msg(2, _validator_set(lb.vals, proposer, total), "validator_set")
    return bytes(m.b), m.fields
