"""A lenient proto3 decoder of tendermint.types.LightBlock and a restatement of
what the reference does with the decoded value (TEST INFRASTRUCTURE: the
oracle for "what would the reference have decoded, and said" in the tests of
tmv_light_blocks_validate_wire; never imported by the product path).

The decoder adds the validator-set messages to tests/block_wire_ref.py (whose
rules it shares: unknown fields skipped, any order, embedded messages merged,
the last scalar wins, padded varints), from the reference's generated
Unmarshal code (proto/tendermint/types/{types,validator}.pb.go,
proto/tendermint/crypto/keys.pb.go): a oneof member that occurs again
replaces the earlier one, whatever its kind; pointer messages (signed_header,
validator_set, header, commit, proposer) are nil until their field occurs.

decode_light_block returns a Decoded, or raises DecodeError where Unmarshal
fails.  from_proto_failure names what LightBlockFromProto
(types/light.go:104-128) does with it that is no ValidateBasic verdict: an
error of PubKeyFromProto or ValidatorFromProto(nil), or updateTotalVotingPower's
panic.  validate_basic is LightBlock.ValidateBasic(chain_id)
(types/light.go:37-60) with ValidatorSet.ValidateBasic
(types/validator_set.go:82-98) and Validator.ValidateBasic
(types/validator.go:74-91).  hashlib and the oracle modules only.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import block_wire_ref as D
import chain_fixtures as CF
import light_ref as L
import merkle_ref as M
from block_wire_ref import DecodeError  # noqa: F401  (re-exported)
from tendermint_amd import host as H

MAX_TOTAL_VOTING_POWER = ((1 << 63) - 1) // 8
KEY_OF_FIELD = {1: H.TMV_KIND_ED25519, 2: 3, 3: 1}  # oneof field -> TMV_KIND_* (secp256k1 = 3, sr25519 = 1)
FIELD_OF_KIND = {v: k for k, v in KEY_OF_FIELD.items()}
KEY_SIZE = {H.TMV_KIND_ED25519: 32, 3: 33, 1: 32}


@dataclass
class DValidator:
    address: bytes = b""
    key_kind: Optional[int] = None  # None: the oneof is unset
    pub_key: bytes = b""
    voting_power: int = 0
    proposer_priority: int = 0


@dataclass
class DValidatorSet:
    validators: List[DValidator] = field(default_factory=list)
    proposer: Optional[DValidator] = None
    total_voting_power: int = 0


@dataclass
class Decoded:
    has_signed_header: bool = False
    header: Optional[H.Header] = None
    commit: Optional[H.Commit] = None
    vals: Optional[DValidatorSet] = None


def _validator(b, lo, hi, v: DValidator):
    for num, x in D._fields(b, lo, hi, {1: 2, 2: 2, 3: 0, 4: 0}):
        if num == 1:
            v.address = b[x[0]:x[1]]
        elif num == 2:
            for n2, x2 in D._fields(b, x[0], x[1], {1: 2, 2: 2, 3: 2}):
                v.key_kind, v.pub_key = KEY_OF_FIELD[n2], b[x2[0]:x2[1]]
        elif num == 3:
            v.voting_power = D._i64(x)
        else:
            v.proposer_priority = D._i64(x)


def _validator_set(b, lo, hi, vs: DValidatorSet):
    for num, x in D._fields(b, lo, hi, {1: 2, 2: 2, 3: 0}):
        if num == 1:
            v = DValidator()
            _validator(b, x[0], x[1], v)
            vs.validators.append(v)
        elif num == 2:
            if vs.proposer is None:
                vs.proposer = DValidator()
            _validator(b, x[0], x[1], vs.proposer)
        else:
            vs.total_voting_power = D._i64(x)


def decode_light_block(b: bytes) -> Decoded:
    d = Decoded()
    for num, x in D._fields(b, 0, len(b), {1: 2, 2: 2}):
        if num == 1:
            d.has_signed_header = True
            for n2, x2 in D._fields(b, x[0], x[1], {1: 2, 2: 2}):
                if n2 == 1:
                    if d.header is None:
                        d.header = H.Header("", 0, H.ZERO_TIME, H.BlockID(), version_block=0, version_app=0)
                    D._header(b, x2[0], x2[1], d.header)
                else:
                    if d.commit is None:
                        d.commit = H.Commit(0, 0, H.BlockID(), [])
                    D._commit(b, x2[0], x2[1], d.commit)
        else:
            if d.vals is None:
                d.vals = DValidatorSet()
            _validator_set(b, x[0], x[1], d.vals)
    return d


def _key_error(v: DValidator) -> bool:
    return v.key_kind is None or len(v.pub_key) != KEY_SIZE[v.key_kind]


def from_proto_failure(d: Decoded) -> Optional[str]:
    """"KEY" / "PROPOSER" / "POWER" where LightBlockFromProto fails or panics
    without it being a ValidateBasic verdict, in the reference's order (every
    key, then the proposer, then the sum of the powers); None where it comes as
    far as ValidateBasic.  The scanner reports the first problem in byte order,
    not in this order: with two faults in one set the two names can differ,
    and both mean "not handled"."""
    vs = d.vals
    if vs is None:
        return None
    for v in vs.validators:
        if _key_error(v):
            return "KEY"
    if vs.proposer is None:
        return "PROPOSER"
    if _key_error(vs.proposer):
        return "KEY"
    total = 0
    for v in vs.validators:  # safeAddClip, types/validator_set.go:888-897
        total = max(-(1 << 63), min((1 << 63) - 1, total + v.voting_power))
        if total > MAX_TOTAL_VOTING_POWER:
            return "POWER"
    return None


def simple_validator_bytes(v) -> bytes:
    """SimpleValidator{pub_key, voting_power}.Marshal() (types/validator.go:154-170)."""
    pub = bytes([(FIELD_OF_KIND[v.key_kind] << 3) | 2, len(v.pub_key)]) + v.pub_key
    out = bytes([0x0A, len(pub)]) + pub
    if v.voting_power:
        out += b"\x10" + M._varint(v.voting_power & ((1 << 64) - 1))
    return out


def vals_hash(validators) -> bytes:
    """ValidatorSet.Hash (types/validator_set.go:344-350)."""
    return M.hash_from_byte_slices([simple_validator_bytes(v) for v in validators])


def header_hash(h: Optional[H.Header]) -> Optional[bytes]:
    return None if h is None else L.header_hash(CF.header(h))


def validator_validate_basic(v: Optional[DValidator]) -> Optional[str]:
    if v is None:
        return "nil validator"
    if v.key_kind is None:
        return "validator does not have a public key"
    if v.voting_power < 0:
        return "validator has negative voting power"
    if len(v.address) != 20:
        return "validator address is the wrong size: " + L.hexu(v.address)
    return None


def valset_validate_basic(vs: Optional[DValidatorSet]) -> Optional[str]:
    if vs is None or not vs.validators:
        return "validator set is nil or empty"
    for i, v in enumerate(vs.validators):
        e = validator_validate_basic(v)
        if e:
            return "invalid validator #%d: %s" % (i, e)
    e = validator_validate_basic(vs.proposer)
    if e:
        return "proposer failed validate basic, error: " + e
    return None


def validate_basic(d: Decoded, chain_id: str) -> Optional[str]:
    if not d.has_signed_header:
        return "missing signed header"
    if d.vals is None:
        return "missing validator set"
    sh = L.SignedHeader(None if d.header is None else CF.header(d.header),
                        None if d.commit is None else CF.commit(d.commit))
    e = L.signed_header_validate_basic(sh, chain_id)
    if e:
        return "invalid signed header: " + e
    e = valset_validate_basic(d.vals)
    if e:
        return "invalid validator set: " + e
    vh = vals_hash(d.vals.validators)
    if d.header.validators_hash != vh:
        return "expected validator hash of header to match validator set hash (%s != %s)" % (
            L.hexu(d.header.validators_hash), L.hexu(vh))
    return None


def expected(b: bytes, chain_id: str):
    """What the wire path must say about a light block it handles: (error text
    or None, Header.Hash or None, ValidatorSet.Hash or None).  Raises
    DecodeError where the reference cannot decode, and returns a reason name
    in place of the tuple where LightBlockFromProto fails otherwise."""
    d = decode_light_block(b)
    bad = from_proto_failure(d)
    if bad:
        return bad
    hh = header_hash(d.header) if d.header is not None and d.header.validators_hash else None
    vh = vals_hash(d.vals.validators) if d.vals is not None and d.vals.validators else None
    return validate_basic(d, chain_id), hh, vh
