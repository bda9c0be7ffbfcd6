"""Blocks validated from their protobuf bytes, on the CPU: the strict scanner
(csrc/host/block_wire.h), tmv_blocks_validate_wire's host path and
chains.blocksync_replay_wire through the host layer built without the engine
(tests/native/blockwire, libblockwirehost.so), against the restatement of the
reference (tests/commit_hash_ref.py) and a lenient decoder written from Go's
unmarshal rules (tests/block_wire_ref.py).  The GPU twin is
tests/test_gpu_block_wire.py."""
import ctypes
import dataclasses
import json
import os

import pytest

import block_wire_cases as W
import block_wire_ref as D
import blocks_cases as C
import commit_hash_ref as R
import mbt_fixtures as MBT
import merkle_ref as M
from tendermint_amd import chains, host as H
from tendermint_amd.testing.block_wire import Field, encode_block, field
from tendermint_amd.testing.blocks import make_full_chain

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libblockwirehost.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "block_wire_vectors.json")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def chain():
    return W.sample_chain(10)


def _strip(b):
    return dataclasses.replace(b, raw=None)


def _golden_block(d):
    def bid(x):
        return H.BlockID(bytes.fromhex(x["hash"]), x["psh_total"], bytes.fromhex(x["psh_hash"]))
    h = d["header"]
    hdr = H.Header(h["chain_id"], h["height"], tuple(h["time"]), bid(h["last_block_id"]),
                   *[bytes.fromhex(h[f]) for f in H._HASH_FIELDS], version_block=h["version"][0],
                   version_app=h["version"][1])
    c = d["last_commit"]
    commit = None if c is None else H.Commit(c["height"], c["round"], bid(c["block_id"]), [
        H.CommitSig(s["flag"], bytes.fromhex(s["address"]), tuple(s["timestamp"]), bytes.fromhex(s["signature"]))
        for s in c["signatures"]])
    return H.FullBlock(hdr, [bytes.fromhex(t) for t in d["txs"]], [], commit)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["vectors"]


@pytest.mark.parametrize("vec", _golden(), ids=lambda v: v["name"])
def test_golden_vectors_pin_encoder_decoder_and_scanner(lib, vec):
    """Bytes written out by hand: the encoder makes them, both decoders read
    them back, and the wire path gives the recorded hashes."""
    block, wire = _golden_block(vec["block"]), bytes.fromhex(vec["wire"])
    got, fs = encode_block(block)
    assert got == wire
    for path, (tag, at, pos, end) in vec["fields"].items():
        f = field(fs, path)
        assert (f.tag, f.at, f.pos, f.end) == (tag, at, pos, end), path
    assert _strip(D.decode_block(wire)) == block
    assert [_strip(b) for b in H.blocks_parse_wire([wire], lib)] == [block]
    (v,) = H.blocks_validate_wire(None, [wire], vec["part_size"], lib)
    assert (v.result != H.WIRE_NOT_HANDLED, v.reason, v.error) == (True, "NONE", vec["validate_basic"])
    assert v.hash.hex() == vec["header_hash"] == R.block_hash(block).hex()
    assert v.part_set_header == (vec["part_set_header"][0], bytes.fromhex(vec["part_set_header"][1]))
    assert R.txs_hash(block.txs).hex() == vec["data_hash"]


def _span_table(lib, wire):
    """The scanner's spans of one block: (signature, transaction, header) leaves as (pos, len, flags)."""
    lib.bw_block_spans.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_uint32)]
    out, counts = (ctypes.c_uint32 * (3 * 4096))(), (ctypes.c_uint32 * 3)()
    assert lib.bw_block_spans(wire, len(wire), out, 4096, counts) == 0
    rows = [tuple(out[3 * i:3 * i + 3]) for i in range(sum(counts))]
    return rows[:counts[0]], rows[counts[0]:counts[0] + counts[1]], rows[counts[0] + counts[1]:]


@pytest.mark.parametrize("vec", _golden(), ids=lambda v: v["name"])
def test_span_table_layout(lib, vec):
    """The spans are where the field map says, with the wrapper tags of
    cdcEncode, and hashlib over them gives the recorded hashes: what the
    device is asked to hash is right before any device hashes it."""
    import hashlib
    from tendermint_amd._native import TMV_SPAN_PREHASH, TMV_SPAN_TAG
    wire = bytes.fromhex(vec["wire"])
    block, fs = _golden_block(vec["block"]), encode_block(_golden_block(vec["block"]))[1]
    sigs, txs, hdr = _span_table(lib, wire)
    by = {f.path: f for f in fs}
    n_sigs = len(block.last_commit.signatures) if block.last_commit else 0
    assert sigs == [(by["last_commit.signatures[%d]" % i].pos, by["last_commit.signatures[%d]" % i].end -
                     by["last_commit.signatures[%d]" % i].pos, 0) for i in range(n_sigs)]
    assert txs == [(by["data.txs[%d]" % i].pos, len(t), TMV_SPAN_PREHASH) for i, t in enumerate(block.txs)]
    want = []
    for name in ("version", "chain_id", "height", "time", "last_block_id") + H._HASH_FIELDS:
        f = by.get("header." + name)
        if f is None:
            want.append((0, 0, 0))  # absent: the empty leaf
        elif name in ("version", "time", "last_block_id"):
            want.append((f.pos, f.end - f.pos, 0))
        else:
            want.append((f.at, f.end - f.at, TMV_SPAN_TAG | (0x08 if name == "height" else 0x0A)))
    assert hdr == want

    def item(pos, n, flags):
        span = wire[pos:pos + n]
        if flags & TMV_SPAN_PREHASH:
            return hashlib.sha256(span).digest()
        return (bytes([flags & 0xFF]) if flags & TMV_SPAN_TAG else b"") + span
    assert M.hash_from_byte_slices([item(*s) for s in hdr]).hex() == vec["header_hash"]
    assert M.hash_from_byte_slices([item(*s) for s in txs]).hex() == vec["data_hash"]
    if block.last_commit is not None:
        assert M.hash_from_byte_slices([item(*s) for s in sigs]).hex() == vec["commit_hash"]


def test_round_trip(lib, chain):
    """Views equal the originals field by field; verdicts, hashes and
    part-set headers equal the struct path's and the restatement's."""
    _, blocks, _ = chain
    extra = [dataclasses.replace(blocks[3], last_commit=None),                       # a nil commit
             dataclasses.replace(blocks[4], txs=[b"", b"x" * 300, b""]),             # zero-length transactions
             dataclasses.replace(blocks[5], txs=[]),
             dataclasses.replace(blocks[5], header=dataclasses.replace(blocks[5].header, validators_hash=b""))]
    extra = [dataclasses.replace(b, raw=encode_block(b)[0]) for b in extra]
    bl = blocks + extra
    assert any(s.block_id_flag == H.BLOCK_ID_FLAG_ABSENT for b in bl[1:] for s in b.last_commit.signatures)
    assert {len(b.txs) for b in bl} >= {0, 1, 2, 5} and any(b"" in b.txs for b in bl)
    raws = [b.raw for b in bl]
    assert H.blocks_parse_wire(raws, lib) == bl
    got = H.blocks_validate_wire(None, raws, 128, lib, decode=True)
    assert [v.block for v in got] == bl
    assert [W.verdict_pair(v) for v in got] == H.blocks_validate_basic(None, bl, lib) == [W.expected(b) for b in bl]
    assert [v.result for v in got] == [H.WIRE_OK] * len(blocks) + [H.WIRE_INVALID, H.WIRE_INVALID, H.WIRE_INVALID,
                                                                   H.WIRE_OK]
    assert got[-1].hash is None  # an empty ValidatorsHash: Header.Hash is nil, and ValidateBasic does not mind
    assert [v.part_set_header for v in got] == [R.part_set_header(r, 128) for r in raws]
    assert all(v.part_set_header is None for v in H.blocks_validate_wire(None, raws, 0, lib))
    assert H.blocks_validate_wire(None, [], 128, lib) == [] and H.blocks_parse_wire([], lib) == []


def test_validate_basic_mutations(lib):
    """Every Block.ValidateBasic mutation of blocks_cases, applied before
    encoding: the same text from the wire path, the struct path and the
    restatement.  Evidence takes a block out of the wire path."""
    blocks = [b for b in C.window_blocks(40) if not b.evidence]
    mutated, names = list(blocks), {}
    import random
    rng = random.Random(78)
    for name, (fn, text) in C.MUTATIONS.items():
        while True:
            i = rng.randrange(len(blocks))
            sigs = blocks[i].last_commit.signatures
            if i not in names and blocks[i].txs and all(sigs[j].block_id_flag == H.BLOCK_ID_FLAG_COMMIT
                                                        for j in (0, 1, -1)):
                break
        mutated[i], names[i] = fn(blocks[i]), (name, text)
    raws = [encode_block(b)[0] for b in mutated]
    got = H.blocks_validate_wire(None, raws, 0, lib)
    want = [W.expected(b) for b in mutated]
    for i, (name, text) in names.items():
        if mutated[i].evidence:
            assert (got[i].result, got[i].reason) == (H.WIRE_NOT_HANDLED, "EVIDENCE"), name
            assert H.blocks_validate_basic(None, [mutated[i]], lib) == [want[i]] and text in want[i][0]
        else:
            assert text in got[i].error, (name, got[i])
    for i, b in enumerate(mutated):
        if not b.evidence:
            assert W.verdict_pair(got[i]) == want[i], names.get(i)
    assert H.blocks_validate_basic(None, [b for b in mutated if not b.evidence], lib) == \
        [w for b, w in zip(mutated, want) if not b.evidence]


def test_rule_table(lib, chain):
    """One mutation per canonical rule: its reason, no verdict, and the
    blocks around it in the same call untouched."""
    _, blocks, _ = chain
    block = next(b for b in blocks[2:] if b.txs)
    good = [blocks[1].raw, blocks[2].raw]
    want_good = [W.expected(b) for b in blocks[1:3]]
    table = W.rule_mutations(block)
    names = sorted(table)
    raws = []
    for n in names:
        raws += [good[0], table[n][0], good[1]]
    got = H.blocks_validate_wire(None, raws, 128, lib, decode=True)
    for k, n in enumerate(names):
        a, v, b = got[3 * k:3 * k + 3]
        assert (v.result, v.reason, v.error, v.hash, v.block) == (H.WIRE_NOT_HANDLED, table[n][1], None, None, None), n
        assert v.part_set_header == R.part_set_header(table[n][0], 128), n
        assert [W.verdict_pair(a), W.verdict_pair(b)] == want_good and a.result == b.result == H.WIRE_OK, n
    seen = {table[n][1] for n in names}
    assert seen >= set(H.WIRE_REASONS) - {"NONE", "LIMIT"}
    assert sum(n.startswith("unknown_field_in:") for n in names) >= 12
    # the lenient decoder reads most of them: the reference would have gone on
    assert _strip(D.decode_block(table["padded_varint"][0])) == _strip(block)
    assert _strip(D.decode_block(table["unknown_field_in:header.time"][0])) == _strip(block)


def _safety(lib, wire, fs):
    """Every single-byte substitution (3 values per position) in one call."""
    muts, where = [], []
    for p in range(len(wire)):
        for x in (wire[p] ^ 0x01, wire[p] ^ 0x80, (wire[p] + 0x3B) & 0xFF):
            muts.append(wire[:p] + bytes([x]) + wire[p + 1:])
            where.append(p)
    got = H.blocks_validate_wire(None, muts, 64, lib, decode=True)
    handled = [i for i, v in enumerate(got) if v.result != H.WIRE_NOT_HANDLED]
    decoded = []
    for i in handled:
        d = D.decode_block(muts[i])  # DecodeError / HasEvidence here: a verdict on bytes the reference rejects
        assert got[i].block == d, where[i]
        decoded.append(d)
    assert [W.verdict_pair(got[i]) for i in handled] == H.blocks_validate_basic(None, decoded, lib) == \
        [W.expected(d) for d in decoded]
    payload = set(W.payload_positions(fs))
    assert len(payload) > len(wire) // 2
    assert {where[i] for i in handled} >= payload and all(
        got[i].result != H.WIRE_NOT_HANDLED for i in range(len(muts)) if where[i] in payload)
    return len(handled), len(muts)


def test_safety_property(lib, chain):
    """A verdict is only ever given on bytes whose lenient decoding -- what the
    reference would have decoded -- gets the same verdict, text and hash from
    the struct path; substitutions in payload bytes are all handled, so the
    test cannot pass by refusing everything."""
    _, blocks, _ = chain
    small = next(b for b in blocks[2:] if len(b.txs) == 1)
    for b in (small, dataclasses.replace(blocks[3], last_commit=None, txs=[b"ab"])):
        wire, fs = encode_block(b)
        n_handled, n = _safety(lib, wire, fs)
        assert 0 < n_handled < n


def test_truncations(lib, chain):
    """Every truncation is handed back; of a block with a commit, the cut in
    front of last_commit leaves the same block with a nil commit."""
    _, blocks, _ = chain
    nil = dataclasses.replace(blocks[2], last_commit=None)
    wire, _ = encode_block(nil)
    got = H.blocks_validate_wire(None, [wire[:n] for n in range(len(wire))], 0, lib)
    assert all(v.result == H.WIRE_NOT_HANDLED and v.reason in ("TRUNCATED", "MISSING") for v in got)
    wire, fs = encode_block(blocks[2])
    cut = field(fs, "last_commit").tag
    got = H.blocks_validate_wire(None, [wire[:n] for n in range(len(wire))], 0, lib, decode=True)
    assert [n for n, v in enumerate(got) if v.result != H.WIRE_NOT_HANDLED] == [cut]
    assert _strip(got[cut].block) == _strip(nil) and got[cut].error == "nil LastCommit"


def test_argument_errors(lib):
    H._setup_block_wire(lib)
    off = (ctypes.c_uint32 * 2)(0, 4)
    res = (ctypes.c_int32 * 1)()
    views = ctypes.c_void_p()
    assert lib.tmv_blocks_validate_wire(None, None, off, 1, 0, res, res, None, 0, None, None, None, None, None) < 0
    data = (ctypes.c_uint8 * 4)()
    assert lib.tmv_blocks_validate_wire(None, data, off, 1, 0, None, res, None, 0, None, None, None, None, None) < 0
    assert lib.tmv_blocks_validate_wire(None, data, off, 1, 64, res, res, None, 0, None, None, None, None, None) < 0
    bad = (ctypes.c_uint32 * 3)(0, 4, 2)
    assert lib.tmv_blocks_parse_wire(data, bad, 2, None, ctypes.byref(views)) < 0 and not views
    assert lib.tmv_blocks_parse_wire(data, off, 1, None, None) < 0
    assert not lib.tmv_block_views_block(None, 0)
    lib.tmv_block_views_free(None)


def test_mbt_header_hashes_through_the_wire_path(lib):
    """The one pin on reference data: the headers of light/mbt/json, encoded,
    must hash to the Go-made header hashes their commits carry."""
    pairs = []
    for case in MBT.load_host_cases():
        for sh in [case["trusted"]] + [i["signed_header"] for i in case["inputs"]]:
            if sh.commit.block_id.hash and sh.header.validators_hash:
                pairs.append((sh.header, sh.commit.block_id.hash))
    assert len(pairs) > 20
    raws = [encode_block(H.FullBlock(h, [], [], None))[0] for h, _ in pairs]
    got = H.blocks_validate_wire(None, raws, 0, lib)
    want = R.block_hash
    agree = [(v.hash, w) for v, (h, w) in zip(got, pairs) if want(H.FullBlock(h)) == w]
    assert len(agree) > 20 and all(v.reason == "NONE" for v in got)
    assert all(a == b for a, b in agree)
    # headers whose recorded hash is another header's (the MBT attack cases) still hash as the restatement says
    assert [v.hash for v in got] == [want(H.FullBlock(h)) for h, _ in pairs]


# ---- the driver ----
@pytest.fixture(scope="module")
def fake():
    import commit_fixtures as F
    fb = F.FakeBackend()
    fb.real_signatures(True)
    yield fb
    fb.real_signatures(False)


@pytest.fixture(scope="module")
def replay_chain():
    vals, blocks, ids = make_full_chain(12, 4, C.CHAIN, seed=41, part_size=128, txs=(1, 4), wire=True)
    return vals, blocks, ids, C.SigCache()


@pytest.mark.parametrize("window,depth", [(1, 1), (5, 2), (100, 1)])
def test_blocksync_replay_wire(lib, fake, replay_chain, window, depth):
    """The replay scenarios of blocks_cases, each block re-encoded after its
    mutation: the wire driver, the struct driver on the decoded blocks and the
    one-at-a-time restatement agree."""
    import commit_fixtures as F
    vals, blocks, ids, cache = replay_chain
    vh = M.validator_set_hash([(v.pub_key, v.key_kind, v.voting_power) for v in vals.validators])
    kw = dict(window=window, depth=depth, part_size=128, verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs),
              lib=lib, vals_hash=vh)
    seen = set()
    for name, (bl, last, height, (applied, at, _)) in C.replay_scenarios(blocks, ids, 7).items():
        if name == "wrong_raw_length":  # raw + one byte is no canonical block: below
            continue
        bl = [dataclasses.replace(b, raw=encode_block(b)[0]) for b in bl]
        want = C.oracle_replay(cache, vals, bl, last, last_block_height=height, part_size=128)
        assert want[0] == applied and (want[1] is None) == (at is None), (name, want)
        assert chains.blocksync_replay_full(None, C.CHAIN, vals, bl, last, last_block_height=height, **kw) == want
        assert chains.blocksync_replay_wire(None, C.CHAIN, vals, [b.raw for b in bl], last, last_block_height=height,
                                            **kw) == want, name
        seen.add(want[1] and want[1][1].split(".")[0].split(" ")[0])
    assert len(seen) >= 2


def test_blocksync_replay_wire_reports_validate_basic(lib, fake):
    """A block that is wrong and properly signed: Block.ValidateBasic's text."""
    import commit_fixtures as F
    edit = {6: lambda h: dataclasses.replace(h, data_hash=C._flip(h.data_hash))}
    vals, blocks, ids = make_full_chain(9, 4, C.CHAIN, seed=42, part_size=128, txs=(1, 3), wire=True, header_edit=edit)
    vh = M.validator_set_hash([(v.pub_key, v.key_kind, v.voting_power) for v in vals.validators])
    kw = dict(part_size=128, verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs), lib=lib, vals_hash=vh)
    want = C.oracle_replay(C.SigCache(), vals, blocks, H.BlockID(), part_size=128)
    assert want[0] == 5 and want[1][0] == 6 and want[1][1].startswith("wrong Header.DataHash. Expected ")
    assert chains.blocksync_replay_wire(None, C.CHAIN, vals, [b.raw for b in blocks], H.BlockID(), **kw) == want
    assert chains.blocksync_replay_full(None, C.CHAIN, vals, blocks, H.BlockID(), **kw) == want


@pytest.mark.parametrize("window", [1, 4, 100])
def test_blocksync_replay_wire_stops_at_a_block_it_does_not_handle(lib, fake, replay_chain, window):
    import commit_fixtures as F
    vals, blocks, ids, _ = replay_chain
    vh = M.validator_set_hash([(v.pub_key, v.key_kind, v.voting_power) for v in vals.validators])
    raws = [b.raw for b in blocks]
    raws[6] = raws[6] + b"\0"  # height 7 with a byte behind it (blocks_cases' wrong_raw_length): field number 0
    got = chains.blocksync_replay_wire(None, C.CHAIN, vals, raws, H.BlockID(), window=window, part_size=128,
                                       verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs), lib=lib,
                                       vals_hash=vh)
    # the pair (6, 7) needs block 7's last commit: the replay ends there, five blocks applied
    assert got == (5, (7, "block wire not handled: UNKNOWN_FIELD"))
    raws = [b.raw for b in blocks]
    raws[0] = raws[0][:-1]
    assert chains.blocksync_replay_wire(None, C.CHAIN, vals, raws, H.BlockID(), window=window, part_size=128,
                                        verify_commits=lambda jobs: [None] * len(jobs), lib=lib, vals_hash=vh) == \
        (0, (1, "block wire not handled: TRUNCATED"))
