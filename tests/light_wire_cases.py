"""Inputs shared by the CPU and the GPU tests of tmv_light_blocks_validate_wire
(tests/test_light_wire_host.py, tests/test_gpu_light_wire.py): a window of
light blocks with their canonical bytes, one mutation per reachable text of
LightBlock.ValidateBasic, the light blocks that the scanner hands back, and
what the restatement (tests/light_wire_ref.py) says about each."""
import dataclasses
import json

import light_wire_ref as R
import mbt_fixtures as MBT
from tendermint_amd import host as H
from tendermint_amd.testing.block_wire import uvarint
from tendermint_amd.testing.factory import _valset_hash, header_hash, make_light_chain
from tendermint_amd.testing.light_wire import encode_light_block, field

CHAIN = "light-wire"
MAX_TOTAL = ((1 << 63) - 1) // 8


def window(n=40, n_vals=7, rotate=1, seed=31):
    """n light blocks over n_vals validators (heights 2 ..), the trusted one in
    front of them, and their canonical bytes."""
    trusted, blocks = make_light_chain(n, n_vals, CHAIN, rotate=rotate, seed=seed)
    return trusted, blocks, [encode_light_block(b)[0] for b in blocks]


def resign(lb, **header_changes):
    """The light block with header fields replaced and the commit's block id
    set to the new header's hash (nothing here reads a signature)."""
    sh = lb.signed_header
    hdr = dataclasses.replace(sh.header, **header_changes)
    bid = dataclasses.replace(sh.commit.block_id, hash=header_hash(hdr))
    return dataclasses.replace(lb, signed_header=H.SignedHeader(hdr, dataclasses.replace(sh.commit, block_id=bid)))


def with_vals(lb, validators, proposer_index=0, fix_header=True):
    """The light block over other validators, its header naming their hash."""
    vs = H.ValidatorSet(list(validators), proposer_index)
    out = dataclasses.replace(lb, vals=vs)
    return resign(out, validators_hash=_valset_hash(vs)) if fix_header and validators else out


def _val(lb, i, **kw):
    vals = list(lb.vals.validators)
    vals[i] = dataclasses.replace(vals[i], **kw)
    return with_vals(lb, vals, lb.vals.proposer_index if lb.vals.proposer_index != i else (i + 1) % len(vals))


def _sh(lb, **kw):
    return dataclasses.replace(lb, signed_header=dataclasses.replace(lb.signed_header, **kw))


def _commit(lb, **kw):
    return _sh(lb, commit=dataclasses.replace(lb.signed_header.commit, **kw))


# name -> (light block -> mutated light block, a piece of the text it must get).
# "proposer failed validate basic" is not here: the proposer's bytes equal an
# entry of `validators` (else PROPOSER), and that entry is reported first.
TEXT_CASES = {
    "missing_signed_header": (lambda b: dataclasses.replace(b, signed_header=None), "missing signed header"),
    "missing_validator_set": (lambda b: dataclasses.replace(b, vals=None), "missing validator set"),
    "missing_header": (lambda b: _sh(b, header=None), "invalid signed header: missing header"),
    "missing_commit": (lambda b: _sh(b, commit=None), "invalid signed header: missing commit"),
    "invalid_header": (lambda b: resign(b, proposer_address=b"\x01" * 19),
                       "invalid signed header: invalid header: invalid ProposerAddress length; got: 19, expected: 20"),
    "invalid_commit": (lambda b: _commit(b, signatures=[]),
                       "invalid signed header: invalid commit: no signatures in commit"),
    "other_chain": (lambda b: resign(b, chain_id="other"),
                    'invalid signed header: header belongs to another chain "other", not "light-wire"'),
    "commit_height": (lambda b: _commit(b, height=b.signed_header.commit.height + 1),
                      "invalid signed header: header and commit height mismatch: "),
    "commit_block_id": (lambda b: _commit(b, block_id=dataclasses.replace(b.signed_header.commit.block_id,
                                                                           hash=b"\x5a" * 32)),
                        "invalid signed header: commit signs block " + "5A" * 32 + ", header is block "),
    "empty_set": (lambda b: with_vals(b, []), "invalid validator set: validator set is nil or empty"),
    "negative_power_0": (lambda b: _val(b, 0, voting_power=-1),
                         "invalid validator set: invalid validator #0: validator has negative voting power"),
    "negative_power_3": (lambda b: _val(b, 3, voting_power=-(1 << 63)),
                         "invalid validator set: invalid validator #3: validator has negative voting power"),
    "address_size_0": (lambda b: _val(b, 0, address=b"\xab" * 19),
                       "invalid validator set: invalid validator #0: validator address is the wrong size: " + "AB" * 19),
    "address_size_4": (lambda b: _val(b, 4, address=b"\xcd" * 21),
                       "invalid validator set: invalid validator #4: validator address is the wrong size: " + "CD" * 21),
    "address_empty_2": (lambda b: _val(b, 2, address=b""),
                        "invalid validator set: invalid validator #2: validator address is the wrong size: "),
    "negative_before_address": (lambda b: _val(_val(b, 1, address=b"\x01"), 5, voting_power=-3),
                                "invalid validator #1: validator address is the wrong size: 01"),
    "validators_hash": (lambda b: resign(b, validators_hash=b"\x77" * 32),
                        "expected validator hash of header to match validator set hash (" + "77" * 32 + " != "),
    "no_validators_hash": (lambda b: resign(b, validators_hash=b""), "invalid signed header: commit signs block "),
}


def encode(lb) -> bytes:
    """The canonical bytes of a (mutated) light block.  An empty set still has
    a proposer on the wire (without one the scanner says PROPOSER)."""
    if lb.vals is not None and not lb.vals.validators:
        return encode_light_block(lb, proposer=H.Validator(b"\x01" * 20, b"\x02" * 32, 1))[0]
    return encode_light_block(lb)[0]


def ld(num: int, payload: bytes) -> bytes:
    """One length-delimited field."""
    return bytes([num << 3 | 2]) + uvarint(len(payload)) + payload


def parts(lb):
    """The payloads of a light block's messages: signed_header, header, commit,
    validator_set, and the Validator messages (entries, then the proposer)."""
    wire, fs = encode_light_block(lb)
    p = {n: wire[field(fs, path).pos:field(fs, path).end]
         for n, path in (("sh", "signed_header"), ("header", "signed_header.header"), ("commit", "signed_header.commit"),
                         ("vs", "validator_set"), ("proposer", "validator_set.proposer"))}
    p["vals"] = [wire[field(fs, "validator_set.validators[%d]" % i).pos:
                      field(fs, "validator_set.validators[%d]" % i).end] for i in range(len(lb.vals.validators))]
    return p


def pointer_cases(lb):
    """Every pointer field absent and present with length 0: name -> (bytes,
    ("INVALID", text) or ("NOT_HANDLED", reason))."""
    p = parts(lb)
    sh, vs = ld(1, p["sh"]), ld(2, p["vs"])
    entries = b"".join(ld(1, v) for v in p["vals"])
    return {
        "signed_header_absent": (vs, ("INVALID", "missing signed header")),
        "signed_header_empty": (ld(1, b"") + vs, ("INVALID", "invalid signed header: missing header")),
        "validator_set_absent": (sh, ("INVALID", "missing validator set")),
        "validator_set_empty": (sh + ld(2, b""), ("NOT_HANDLED", "PROPOSER")),
        "both_absent": (b"", ("INVALID", "missing signed header")),
        "header_absent": (ld(1, ld(2, p["commit"])) + vs, ("INVALID", "invalid signed header: missing header")),
        "header_empty": (ld(1, ld(1, b"") + ld(2, p["commit"])) + vs, ("NOT_HANDLED", "MISSING")),
        "commit_absent": (ld(1, ld(1, p["header"])) + vs, ("INVALID", "invalid signed header: missing commit")),
        "commit_empty": (ld(1, ld(1, p["header"]) + ld(2, b"")) + vs, ("NOT_HANDLED", "MISSING")),
        "proposer_absent": (sh + ld(2, entries), ("NOT_HANDLED", "PROPOSER")),
        "proposer_empty": (sh + ld(2, entries + ld(2, b"")), ("NOT_HANDLED", "MISSING")),
        "validator_entry_empty": (sh + ld(2, ld(1, b"") + entries + ld(2, p["proposer"])), ("NOT_HANDLED", "MISSING")),
    }


def reason_cases(lb):
    """The three light-block reasons: name -> (bytes, reason)."""
    v = lb.vals.validators
    out = {}

    def enc(vals, **kw):
        return encode_light_block(dataclasses.replace(lb, vals=H.ValidatorSet(list(vals), 0)), **kw)[0]
    key = lambda i, **kw: [dataclasses.replace(x, **kw) if j == i else x for j, x in enumerate(v)]  # noqa: E731
    out["key_unset"] = (enc(key(0, key_kind=H.KIND_OTHER)), "KEY")
    out["key_unset_later"] = (enc(key(3, key_kind=H.KIND_OTHER)), "KEY")
    out["key_ed25519_31"] = (enc(key(1, pub_key=b"\x01" * 31)), "KEY")
    out["key_ed25519_33"] = (enc(key(1, pub_key=b"\x01" * 33)), "KEY")
    out["key_ed25519_empty"] = (enc(key(2, pub_key=b"")), "KEY")
    out["key_secp256k1_32"] = (enc(key(2, pub_key=b"\x02" * 32, key_kind=3)), "KEY")
    out["key_secp256k1_34"] = (enc(key(2, pub_key=b"\x02" * 34, key_kind=3)), "KEY")
    out["key_sr25519_33"] = (enc(key(0, pub_key=b"\x03" * 33, key_kind=1)), "KEY")
    out["proposer_nil"] = (enc(v, proposer=None), "PROPOSER")
    out["proposer_stranger"] = (enc(v, proposer=dataclasses.replace(v[0], address=b"\x09" * 20)), "PROPOSER")
    out["proposer_other_priority"] = (enc(v, proposer=dataclasses.replace(v[0], proposer_priority=5)), "PROPOSER")
    out["power_one"] = (enc(key(0, voting_power=MAX_TOTAL + 1)), "POWER")
    out["power_sum"] = (enc(key(0, voting_power=MAX_TOTAL) + [dataclasses.replace(v[1], address=b"\x08" * 20)]), "POWER")
    out["power_clipped"] = (enc([dataclasses.replace(x, voting_power=(1 << 63) - 1) for x in v[:2]]), "POWER")
    return out


def verdict(v):
    """(error text, Header.Hash, ValidatorSet.Hash) of a handled LightWireVerdict, as R.expected gives it."""
    return v.error, v.hash, v.vals_hash


def expected(raw: bytes, chain_id: str = CHAIN):
    return R.expected(raw, chain_id)


def mbt_light_blocks():
    """(file, host.LightBlock) of every input of tests/golden/mbt_light.json: Go-made
    validator sets, ValidatorsHash, header hashes and commits."""
    with open(MBT.GOLDEN) as f:
        data = json.load(f)
    out = []
    for c in data["cases"]:
        for inp in c["input"]:
            out.append((c["file"], H.LightBlock(MBT.host_signed_header(inp["signed_header"]),
                                                MBT.host_valset(inp["validator_set"]))))
    return out


EMPTY_SET_INPUT = ("light/mbt/json/MC4_4_faulty_TestUntrustedBeforeTrusted.json", 4)  # (file, height)


def go_made_light_blocks():
    """The inputs of mbt_light.json split by their data alone, not by anything
    computed here: (the 29 whose validator set is not empty, the one whose set
    is empty -- EMPTY_SET_INPUT, which the model made so)."""
    full = [(f, lb) for f, lb in mbt_light_blocks() if lb.vals.validators]
    rest = [(f, lb) for f, lb in mbt_light_blocks() if not lb.vals.validators]
    assert len(full) == 29 and [(f, lb.height) for f, lb in rest] == [EMPTY_SET_INPUT]
    return [lb for _, lb in full], [lb for _, lb in rest]
