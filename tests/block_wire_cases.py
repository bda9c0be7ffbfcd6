"""Cases shared by the CPU and GPU tests of the block wire path
(tmv_blocks_validate_wire, chains.blocksync_replay_wire): byte-level mutations
made from the encoder's field map, one per canonical rule, and the expected
verdicts from the restatement of the reference (tests/commit_hash_ref.py)."""
import dataclasses

import blocks_cases as C
import commit_hash_ref as R
from tendermint_amd import host as H
from tendermint_amd.testing.block_wire import encode_block, field, uvarint
from tendermint_amd.testing.blocks import make_full_chain


def splice(wire: bytes, fields, msg_path: str, lo: int, hi: int, ins: bytes) -> bytes:
    """wire with wire[lo:hi], which lies in the message at msg_path ("" = the
    block), replaced by ins, and the length of that message and of every
    message around it written anew."""
    around = [f for f in fields if msg_path and (f.path == msg_path or msg_path.startswith(f.path + "."))]
    cur_lo, cur_hi, cur = lo, hi, ins
    for f in sorted(around, key=lambda f: f.end - f.pos):
        payload = wire[f.pos:cur_lo] + cur + wire[cur_hi:f.end]
        cur, cur_lo, cur_hi = uvarint(len(payload)) + payload, f.at, f.end
    return wire[:cur_lo] + cur + wire[cur_hi:]


def parent(path: str) -> str:
    return path.rpartition(".")[0]


def expected(block):
    """What blocks_validate_wire must say of a handled block: (text, hash)."""
    return R.block_validate_basic(block), R.block_hash(block)


def verdict_pair(v):
    return v.error, v.hash


def sample_chain(n=8, seed=61, **kw):
    """Small signed blocks with their real encoding as `raw`: nil-free commits
    with one absent signature, 0..5 transactions, a zero-length transaction."""
    vals, blocks, ids = make_full_chain(n, 4, C.CHAIN, seed=seed, part_size=128, txs=(0, 5), tx_len=(0, 40),
                                        absent=(2,), wire=True, **kw)
    return vals, blocks, ids


def unknown_field_paths(fields):
    """Every message of a block an unknown field can be appended to: the block
    itself and each embedded message but the evidence list (anything in it
    is evidence)."""
    out = [""]
    for f in fields:
        leaf = f.path.rpartition(".")[2]
        if f.wire_type == 2 and f.path != "evidence" and (
                leaf in ("header", "version", "time", "last_block_id", "part_set_header", "data", "last_commit",
                         "block_id", "timestamp") or leaf.startswith("signatures[")):
            out.append(f.path)
    return out


def rule_mutations(block):
    """name -> (bytes, reason name): one mutation per canonical rule of a block
    that has a commit with signatures and at least one transaction."""
    T0 = block.header.time[0]
    wire, fs = encode_block(block)
    f = lambda p: field(fs, p)
    cid, hgt, tim, prop = f("header.chain_id"), f("header.height"), f("header.time"), f("header.proposer_address")
    lch = f("last_commit.height")
    out = {}
    out["fields_swapped"] = (wire[:cid.tag] + wire[hgt.tag:hgt.end] + wire[cid.tag:cid.end] + wire[hgt.end:], "ORDER")
    out["scalar_twice"] = (splice(wire, fs, "header", hgt.end, hgt.end, wire[hgt.tag:hgt.end]), "ORDER")
    out["embedded_message_twice"] = (splice(wire, fs, "header", tim.end, tim.end, wire[tim.tag:tim.end]), "ORDER")
    v = wire[hgt.at:hgt.end]
    out["padded_varint"] = (splice(wire, fs, "header", hgt.at, hgt.end, v[:-1] + bytes([v[-1] | 0x80, 0])), "VARINT")
    out["padded_length"] = (splice(wire, fs, "header", cid.at, cid.pos,
                                   bytes([wire[cid.at] | 0x80, 0])), "VARINT")
    out["varint_11_bytes"] = (splice(wire, fs, "header", hgt.at, hgt.end, b"\x80" * 10 + b"\x01"), "VARINT")
    out["varint_beyond_64_bits"] = (splice(wire, fs, "header", hgt.at, hgt.end, b"\xff" * 9 + b"\x02"), "VARINT")
    out["negative_int32_in_5_bytes"] = (splice(wire, fs, "last_commit", lch.end, lch.end,
                                               b"\x10\xff\xff\xff\xff\x0f"), "VARINT")
    tot = f("last_commit.block_id.part_set_header.total")
    out["uint32_above_32_bits"] = (splice(wire, fs, "last_commit.block_id.part_set_header", tot.at, tot.end,
                                          b"\x81\x80\x80\x80\x10"), "VARINT")
    out["zero_scalar_present"] = (splice(wire, fs, "last_commit", lch.end, lch.end, b"\x10\x00"), "ZERO_PRESENT")
    app = f("header.app_hash")
    out["empty_bytes_present"] = (splice(wire, fs, "header", app.tag, app.end, b"\x5a\x00"), "ZERO_PRESENT")
    out["header_time_dropped"] = (splice(wire, fs, "header", tim.tag, tim.end, b""), "MISSING")
    ev = f("evidence")
    out["evidence_list_dropped"] = (wire[:ev.tag] + wire[ev.end:], "MISSING")
    ts = f("last_commit.signatures[0].timestamp")
    out["sig_timestamp_dropped"] = (splice(wire, fs, "last_commit.signatures[0]", ts.tag, ts.end, b""), "MISSING")
    psh = f("header.last_block_id.part_set_header")
    out["part_set_header_dropped"] = (splice(wire, fs, "header.last_block_id", psh.tag, psh.end, b""), "MISSING")
    for p in unknown_field_paths(fs):
        end = len(wire) if p == "" else f(p).end
        out["unknown_field_in:" + (p or "block")] = (splice(wire, fs, p, end, end, b"\xf8\x01\x01"), "UNKNOWN_FIELD")
    out["field_number_0"] = (wire + b"\x00\x01", "UNKNOWN_FIELD")
    out["wrong_wire_type"] = (wire[:hgt.tag] + b"\x1a" + wire[hgt.at:], "WIRE_TYPE")
    out["fixed64_for_varint"] = (wire[:hgt.tag] + b"\x19" + wire[hgt.at:], "WIRE_TYPE")
    out["length_past_parent"] = (wire[:prop.at] + bytes([wire[prop.at] + 1]) + wire[prop.pos:], "TRUNCATED")
    out["last_byte_cut"] = (wire[:-1], "TRUNCATED")
    out["empty"] = (b"", "MISSING")
    hdr = block.header
    out["nanos_1e9"] = (encode_block(dataclasses.replace(block, header=dataclasses.replace(
        hdr, time=(T0, 10**9))))[0], "TIME")
    out["seconds_after_9999"] = (encode_block(dataclasses.replace(block, header=dataclasses.replace(
        hdr, time=(253402300800, 0))))[0], "TIME")
    out["negative_nanos"] = (encode_block(C._commit_with(block, 0, timestamp=(T0, -1)))[0], "TIME")
    out["evidence"] = (encode_block(dataclasses.replace(block, evidence=[b"\x0a\x02ev"]))[0], "EVIDENCE")
    out["chain_id_not_ascii"] = (wire[:cid.pos] + b"\xc3" + wire[cid.pos + 1:], "CHAIN_ID")
    out["chain_id_nul"] = (wire[:cid.pos + 1] + b"\x00" + wire[cid.pos + 2:], "CHAIN_ID")
    out["flag_256"] = (encode_block(C._commit_with(block, 0, block_id_flag=256))[0], "LIMIT")
    return out


def payload_positions(fs):
    """Positions of bytes that no canonical rule reads: hashes, addresses,
    signatures and transaction bytes."""
    out = []
    for f in fs:
        leaf = f.path.rpartition(".")[2]
        if f.wire_type == 2 and (leaf in H._HASH_FIELDS or leaf in ("hash", "validator_address", "signature") or
                                 leaf.startswith("txs[")):
            out += range(f.pos, f.end)
    return out
