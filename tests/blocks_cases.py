"""Cases shared by the CPU and GPU tests of the block layer (Commit.Hash,
Block.ValidateBasic, blocksync_replay_full): the CommitSig encoder cases, the
ValidateBasic mutations and the replay scenarios, each compared for exact
equality with tests/commit_hash_ref.py."""
import copy
import dataclasses
import random

import chain_fixtures as CF
import commit_hash_ref as R
import ed25519_ref
import light_ref as L
from tendermint_amd import host as H
from tendermint_amd.testing.blocks import make_full_chain

CHAIN = "test_chain_id"
ADDR = bytes(range(1, 21))
SIG = bytes((7 * i + 3) & 0xFF for i in range(64))
ZERO_SECS = -62135596800
T = 1577836800

# (flag, address, seconds, nanos, signature)
ENCODER_CASES = {
    "absent": (1, b"", ZERO_SECS, 0, b""),
    "flag0": (0, ADDR, T, 5, SIG),
    "flag2": (2, ADDR, T, 5, SIG),
    "flag3": (3, ADDR, T, 5, SIG),
    "flag127": (127, ADDR, T, 5, SIG),
    "secs0": (2, ADDR, 0, 7, SIG),
    "nanos0": (2, ADDR, T, 0, SIG),
    "time0": (2, ADDR, 0, 0, SIG),
    "secs-1": (2, ADDR, -1, 1, SIG),
    "secs_zero_time": (2, ADDR, ZERO_SECS, 3, SIG),
    "secs_max": (2, ADDR, 253402300799, 0, SIG),
    "nanos_max": (2, ADDR, T, 999999999, SIG),
    "longest": (2, ADDR, ZERO_SECS, 999999999, SIG),
    "sig0": (2, ADDR, T, 5, b""),
    "sig1": (2, ADDR, T, 5, SIG[:1]),
    "sig63": (2, ADDR, T, 5, SIG[:63]),
    "sig64": (2, ADDR, T, 5, SIG),
    "no_addr": (3, b"", T, 5, SIG),
}
# with a 20-byte address, seconds = T and nanos = 0 the leaf with its prefix is
# 35 + len(sig) bytes: the SHA-256 block boundaries
BOUNDARY = {20: 55, 21: 56, 28: 63, 29: 64, 30: 65}
for _n in BOUNDARY:
    ENCODER_CASES["leaf%d" % BOUNDARY[_n]] = (2, ADDR, T, 0, SIG[:_n])


# outside the reference's domain (StdTimeMarshalTo fails there): encoded as plain protobuf int64 / int32
OUT_OF_DOMAIN_CASES = {
    "nanos-1": (2, ADDR, T, -1, SIG),
    "nanos_1e9": (2, ADDR, T, 10**9, SIG),
    "secs_after_9999": (2, ADDR, 253402300800, 1, SIG),
    "secs_min": (2, ADDR, -(1 << 63), -(1 << 31), SIG),  # the longest leaf there is: 115 bytes
    "secs_max_i64": (3, b"", (1 << 63) - 1, (1 << 31) - 1, b""),
}


def check_case_lengths():
    assert len(b"\0" + R.commit_sig_bytes(*OUT_OF_DOMAIN_CASES["secs_min"])) == 115
    assert len(b"\0" + R.commit_sig_bytes(*ENCODER_CASES["absent"])) == 16
    assert len(b"\0" + R.commit_sig_bytes(*ENCODER_CASES["longest"])) == 110
    assert R.commit_sig_bytes(*ENCODER_CASES["time0"])[24:26] == b"\x1a\x00"
    for n, want in BOUNDARY.items():
        assert len(b"\0" + R.commit_sig_bytes(*ENCODER_CASES["leaf%d" % want])) == want
    for flag, addr, secs, nanos, sig in ENCODER_CASES.values():  # inside the reference's domain
        assert R.timestamp_bytes(secs, nanos) == L.proto_timestamp(secs * L.NS + nanos)


def random_sig(rng: random.Random):
    flag = rng.choice([0, 1, 2, 2, 2, 3, 127])
    addr = bytes(rng.randrange(256) for _ in range(20)) if rng.random() < 0.8 else b""
    secs = rng.choice([0, -1, ZERO_SECS, T + rng.randrange(10**6), rng.randrange(ZERO_SECS, 253402300800)])
    nanos = rng.choice([0, rng.randrange(10**9)])
    sig = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 20, 21, 28, 29, 30, 63, 64, 64, 64])))
    return flag, addr, secs, nanos, sig


def columns(commits):
    """tmv_commit_hashes' column arrays for commits = [[(flag, addr, secs, nanos, sig)]]."""
    import numpy as np
    sigs = [s for c in commits for s in c]
    n = len(sigs)
    flag = np.array([s[0] for s in sigs], np.uint8)
    addr_len = np.array([len(s[1]) for s in sigs], np.uint8)
    addr = np.zeros((n, 20), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    for i, s in enumerate(sigs):
        addr[i, :len(s[1])] = np.frombuffer(s[1], np.uint8)
        sig[i, :len(s[4])] = np.frombuffer(s[4], np.uint8)
    secs = np.array([s[2] for s in sigs], np.int64)
    nanos = np.array([s[3] for s in sigs], np.int32)
    sig_len = np.array([len(s[4]) for s in sigs], np.uint8)
    off = np.zeros(len(commits) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in commits])
    return flag, addr_len, addr, secs, nanos, sig_len, sig, off


def host_commit(sigs, height=5):
    return H.Commit(height, 0, H.BlockID(b"\x11" * 32, 1, b"\x22" * 32),
                    [H.CommitSig(f, a, (s, ns), sg) for f, a, s, ns, sg in sigs])


# ---- Block.ValidateBasic mutations: name -> (function on a copy of the block, substring of the text) ----
def _flip(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


def _hdr(b, **kw):
    return dataclasses.replace(b, header=dataclasses.replace(b.header, **kw))


def _commit_with(b, i, **kw):
    c = copy.deepcopy(b.last_commit)
    c.signatures[i] = dataclasses.replace(c.signatures[i], **kw)
    return dataclasses.replace(b, last_commit=c)


def _ts_tamper(b, i=-1):
    s = b.last_commit.signatures[i]
    return _commit_with(b, i, timestamp=(s.timestamp[0], s.timestamp[1] + 1))


MUTATIONS = {
    "last_commit_hash_tampered": (lambda b: _hdr(b, last_commit_hash=_flip(b.header.last_commit_hash)),
                                  "wrong Header.LastCommitHash. Expected "),
    "data_hash_tampered": (lambda b: _hdr(b, data_hash=_flip(b.header.data_hash)), "wrong Header.DataHash. Expected "),
    "evidence_hash_tampered": (lambda b: _hdr(b, evidence_hash=_flip(b.header.evidence_hash)),
                               "wrong Header.EvidenceHash. Expected "),
    "last_commit_hash_empty": (lambda b: _hdr(b, last_commit_hash=b""), "wrong Header.LastCommitHash. Expected "),
    "data_hash_empty": (lambda b: _hdr(b, data_hash=b""), "wrong Header.DataHash. Expected "),
    "evidence_hash_empty": (lambda b: _hdr(b, evidence_hash=b""), "wrong Header.EvidenceHash. Expected "),
    "nil_commit": (lambda b: dataclasses.replace(b, last_commit=None), "nil LastCommit"),
    "bad_commit_sig": (lambda b: _commit_with(b, 1, signature=b""),
                       "wrong LastCommit: wrong CommitSig #1: signature is missing"),
    "bad_header_proposer": (lambda b: _hdr(b, proposer_address=b.header.proposer_address[:19]),
                            "invalid header: invalid ProposerAddress length; got: 19, expected: 20"),
    "bad_header_version": (lambda b: _hdr(b, version_block=10), "invalid header: block protocol is incorrect"),
    "tx_tampered": (lambda b: dataclasses.replace(b, txs=[_flip(b.txs[0])] + b.txs[1:]),
                    "wrong Header.DataHash. Expected "),
    "tx_appended": (lambda b: dataclasses.replace(b, txs=b.txs + [b"x"]), "wrong Header.DataHash. Expected "),
    "commit_sig_time_tampered": (_ts_tamper, "wrong Header.LastCommitHash. Expected "),
    "evidence_tampered": (lambda b: dataclasses.replace(b, evidence=b.evidence + [b"ev"]),
                          "wrong Header.EvidenceHash. Expected "),
    # a block failing an earlier check reports that check, not a later one
    "header_before_nil_commit": (lambda b: dataclasses.replace(_hdr(b, height=0), last_commit=None),
                                 "invalid header: zero Height"),
    "commit_before_hashes": (lambda b: _hdr(_commit_with(b, 0, signature=b"\1" * 65), data_hash=b""),
                             "wrong LastCommit: wrong CommitSig #0: signature is too big (max: 64)"),
    "commit_hash_before_data": (lambda b: _hdr(_ts_tamper(b), data_hash=_flip(b.header.data_hash)),
                                "wrong Header.LastCommitHash. Expected "),
    "data_before_evidence": (lambda b: _hdr(b, data_hash=_flip(b.header.data_hash),
                                            evidence_hash=_flip(b.header.evidence_hash)),
                             "wrong Header.DataHash. Expected "),
}


def window_blocks(n=40, seed=5):
    """n small blocks: 3 to 9 signatures (validators absent at random), 0 to 5
    transactions, two evidence items in one block.  Unsigned: ValidateBasic
    reads no signature."""
    rng = random.Random(seed)
    out = []
    for k, nv in enumerate([3, 4, 5, 6, 7, 8, 9]):
        _, blocks, _ = make_full_chain((n + 6) // 7 + 1, nv, CHAIN, seed=seed + k, raw_len=(1, 64), txs=(0, 5),
                                       tx_len=(1, 200), evidence_at={3: [b"evidence-one", b"e2" * 40]} if k == 2 else None,
                                       absent=rng.sample(range(nv), rng.randrange(0, 2)), sign=False)
        out += blocks[1:]  # height 1 carries no signatures
    rng.shuffle(out)
    out = out[:n]
    assert any(len(b.evidence) == 2 for b in out) and any(not b.txs for b in out)
    return out


def check_validate_basic(ctx, lib, blocks):
    """The window clean, then every mutation applied to one block each."""
    want = [(R.block_validate_basic(b), R.block_hash(b)) for b in blocks]
    assert all(e is None for e, _ in want)
    assert H.blocks_validate_basic(ctx, blocks, lib) == want
    rng = random.Random(77)
    mutated = list(blocks)
    expect_text = {}
    for name, (fn, text) in MUTATIONS.items():
        while True:
            i = rng.randrange(len(blocks))
            b = blocks[i]
            sigs = b.last_commit.signatures
            if i not in expect_text and len(b.txs) >= 1 and \
                    all(sigs[j].block_id_flag == H.BLOCK_ID_FLAG_COMMIT for j in (0, 1, -1)):
                break
        mutated[i] = fn(b)
        expect_text[i] = (name, text)
    want = [(R.block_validate_basic(b), R.block_hash(b)) for b in mutated]
    for i, (name, text) in expect_text.items():
        assert want[i][0] is not None and text in want[i][0], (name, want[i][0])
    got = H.blocks_validate_basic(ctx, mutated, lib)
    assert got == want
    assert sum(e is not None for e, _ in got) == len(MUTATIONS)


# ---- blocksync_replay_full ----
class SigCache:
    """light_ref signature verdicts, each computed once (a commit is read light
    at height H and full at H + 1)."""

    def __init__(self):
        self.m = {}

    def __call__(self, v, msg, sig):
        key = (v.pub_key, msg, sig)
        if key not in self.m:
            self.m[key] = len(sig) == 64 and ed25519_ref.verify_zip215(v.pub_key, msg, sig)
        return self.m[key]


def oracle_replay(cache, vals, blocks, last_block_id, **kw):
    ov = CF.valset(vals)

    def text(e):
        return None if e is None else e.text

    def light(bid, height, commit):
        return text(L.verify_commit_light(CHAIN, ov, CF.block_id(bid), height,
                                          None if commit is None else CF.commit(commit)))

    def full(bid, height, commit):
        return text(L.verify_commit(CHAIN, ov, CF.block_id(bid), height, None if commit is None else CF.commit(commit)))

    with L.signature_oracle(cache):
        return R.replay_full(CHAIN, vals, blocks, last_block_id, light, full, ov.hash(), **kw)


def replay_scenarios(blocks, ids, k):
    """name -> (blocks, last_block_id, last_block_height, (applied, height, substring) wanted), k = the
    height that fails (block index k - 1)."""
    i = k - 1
    out = {"clean": (blocks, H.BlockID(), 0, (len(blocks) - 1, None, None))}
    b = list(blocks)
    b[i] = MUTATIONS["tx_tampered"][0](blocks[i]) if blocks[i].txs else MUTATIONS["tx_appended"][0](blocks[i])
    out["tx_tampered"] = (b, H.BlockID(), 0, (i, k, "wrong Header.DataHash. Expected "))
    b = list(blocks)
    b[i] = _ts_tamper(blocks[i])  # the last signature: VerifyCommitLight at k - 1 stops before it
    out["commit_sig_time_tampered"] = (b, H.BlockID(), 0, (i, k, "wrong Header.LastCommitHash. Expected "))
    out["wrong_last_block_id"] = (blocks[i:], H.BlockID(b"\x07" * 32, 1, b"\x08" * 32), k - 1,
                                  (0, k, "wrong Block.Header.LastBlockID.  Expected " + "07" * 32 + ":1:080808080808, got "))
    b = list(blocks)
    b[i] = dataclasses.replace(blocks[i], raw=blocks[i].raw + b"\0")
    out["wrong_raw_length"] = (b, H.BlockID(), 0, (i, k, "invalid commit -- wrong block ID: want "))
    return out


def check_replay(run, cache, vals, blocks, ids, k, names=None, part_size=65536):
    """run(blocks, last_block_id, last_block_height) -> blocksync_replay_full's result."""
    for name, (bl, last, height, (applied, at, text)) in replay_scenarios(blocks, ids, k).items():
        if names is not None and name not in names:
            continue
        want = oracle_replay(cache, vals, bl, last, last_block_height=height, part_size=part_size)
        assert want[0] == applied, (name, want)
        if at is None:
            assert want[1] is None, (name, want)
        else:
            assert want[1][0] == at and text in want[1][1], (name, want)
        assert run(bl, last, height) == want, name
