"""Cases shared by the CPU and GPU tests of the results layer (the tx-result
encoder, the results roots, both light-client verify calls and
blocksync_replay_stateful), each compared for exact equality with
tests/results_ref.py."""
import dataclasses
import random

import numpy as np

import results_ref as R
from tendermint_amd import chains, host as H
from tendermint_amd.testing.blocks import make_stateful_chain

CHAIN = "test_chain_id"
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def _data(n: int) -> bytes:
    return bytes((31 * i + n) & 0xFF for i in range(n))


# name -> (code, data, gas_wanted, gas_used)
CASES = {"empty": (0, b"", 0, 0)}
for _c in (0, 127, 128, (1 << 32) - 1):
    CASES["code%d" % _c] = (_c, b"", 0, 0)
    CASES["code%d_data" % _c] = (_c, b"abc", 7, 9)
for _g in (0, 1, -1, I64_MAX, I64_MIN):
    CASES["gas_wanted%d" % _g] = (1, b"x", _g, 0)
    CASES["gas_used%d" % _g] = (1, b"x", 0, _g)
    CASES["gas_both%d" % _g] = (0, b"", _g, _g)
for _n in (0, 1, 127, 128, 16383, 16384):
    CASES["data%d" % _n] = (0, _data(_n), 0, 0)
    CASES["data%d_framed" % _n] = (300, _data(_n), -1, 5)
# with no code and no gas the leaf (0x00 || 12 L data) is L + 3 bytes for L < 128: the SHA-256 block boundaries
BOUNDARY = {52: 55, 53: 56, 60: 63, 61: 64, 116: 119, 117: 120, 124: 127, 125: 128}
for _n in BOUNDARY:
    CASES["leaf%d" % BOUNDARY[_n]] = (0, _data(_n), 0, 0)
# a 4-byte head and a 21-byte tail around data of every length from 30 to 70: the tail crosses a block boundary
# at every offset, and the data starts at every alignment
for _n in range(30, 71):
    CASES["tail_cross%d" % _n] = (300, _data(_n), -1, I64_MAX)
CASES["longest_frame"] = ((1 << 32) - 1, _data(16384), I64_MIN, -1)

TREE_SIZES = (0, 1, 2, 3, 64, 65, 128, 129, 257)


def check_case_lengths():
    for n, want in BOUNDARY.items():
        assert len(b"\0" + R.tx_result_bytes(*CASES["leaf%d" % want])) == want
    enc = R.tx_result_bytes(*CASES["longest_frame"])
    assert len(enc) - 16384 == 6 + 4 + 11 + 11  # 08 + 5, 12 + 3, 28 + 10, 30 + 10
    assert R.tx_result_bytes(*CASES["gas_both-1"]) == b"\x28" + b"\xff" * 9 + b"\x01" + b"\x30" + b"\xff" * 9 + b"\x01"
    assert R.tx_result_bytes(*CASES["empty"]) == b""


def tree(n: int, seed: int):
    """n results drawn from the case table (the 16 KiB ones rarely)."""
    rng = random.Random(seed)
    small = [c for c in CASES.values() if len(c[1]) < 1000]
    return [rng.choice(list(CASES.values())) if rng.random() < 0.02 else rng.choice(small) for _ in range(n)]


def columns(trees):
    """tmv_tx_results_hashes' arrays for trees = [[(code, data, gas_wanted, gas_used)]]:
    (code, gas_wanted, gas_used, data, data_off, tree_off)."""
    rs = [r for t in trees for r in t]
    code = np.array([r[0] for r in rs], np.uint32)
    gw = np.array([r[2] for r in rs], np.int64)
    gu = np.array([r[3] for r in rs], np.int64)
    data = np.frombuffer(b"".join(r[1] for r in rs), np.uint8)
    data_off = np.zeros(len(rs) + 1, np.uint32)
    data_off[1:] = np.cumsum([len(r[1]) for r in rs])
    tree_off = np.zeros(len(trees) + 1, np.uint32)
    tree_off[1:] = np.cumsum([len(t) for t in trees])
    return code, gw, gu, data, data_off, tree_off


def first_columns(firsts):
    off = np.zeros(len(firsts) + 1, np.uint32)
    off[1:] = np.cumsum([len(f) for f in firsts])
    return np.frombuffer(b"".join(firsts), np.uint8), off


def host_results(rs):
    return [H.TxResult(*r) for r in rs]


def as_tuples(results):
    return [(r.code, r.data, r.gas_wanted, r.gas_used) for r in results]


# ---- the light client's verify calls ----
def block_results_items():
    """[(host.BlockResults, the text wanted or None)]: ok, both texts, heights 0 and -1."""
    out = []
    for k, n in enumerate((0, 1, 3, 65, 130)):
        rs = tree(n, 100 + k)
        events = _data(17 * k)
        out.append((k + 1, rs, events, R.results_hash(rs, events)))
    rs = tree(5, 7)
    items = [(h, rs_, ev, tr) for h, rs_, ev, tr in out]
    items.append((0, rs, b"ev", R.results_hash(rs, b"ev")))
    items.append((-1, rs, b"ev", R.results_hash(rs, b"ev")))
    items.append((9, rs, b"ev", R.results_hash(rs, None)))            # trusted hash lacks the leading leaf
    items.append((9, rs, b"", R.results_hash(rs, b"")))               # an empty leading leaf is a leaf
    items.append((9, rs, b"ev", R.results_hash(rs, b"ev")[:31]))      # a short trusted hash
    items.append((9, rs[:-1], b"ev", R.results_hash(rs, b"ev")))      # a result missing
    items.append((9, [], b"", b""))                                   # nothing at all against an empty hash
    return [(H.BlockResults(h, host_results(rs_), ev, tr), R.block_results_verify(h, rs_, ev, tr))
            for h, rs_, ev, tr in items]


def consensus_params_items():
    good = R.consensus_params_hash(22020096, -1)
    items = [(5, 22020096, -1, good), (0, 22020096, -1, good), (-1, 22020096, -1, good), (5, 22020097, -1, good),
             (5, 22020096, 0, good), (5, 0, 0, R.consensus_params_hash(0, 0)), (5, 1, 1, R.consensus_params_hash(1, 1)),
             (5, 1, 1, b""), (1, I64_MAX, I64_MIN, R.consensus_params_hash(I64_MAX, I64_MIN))]
    return [(H.ConsensusParamsResult(*it), R.consensus_params_verify(*it)) for it in items]


# ---- blocksync_replay_stateful ----
N_BLOCKS, N_VALS, FAIL_AT = 12, 4, 7
EVIDENCE = [b"evidence-one", b"e2" * 80]  # ByteSize = (1 + 1 + 12) + (1 + 2 + 160) = 177


def _flip(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


def stateful_chain(header_edit=None, evidence_at=None):
    return make_stateful_chain(N_BLOCKS, N_VALS, CHAIN, seed=41, raw_len=(1, 300), part_size=128, txs=(1, 4),
                               header_edit=header_edit, evidence_at=evidence_at)


def _edit(**kw):
    """header_edit for the failing height: fields replaced by value, or by f(old value) for a callable."""
    def fn(h):
        return dataclasses.replace(h, **{k: (v(getattr(h, k)) if callable(v) else v) for k, v in kw.items()})
    return {FAIL_AT: fn}


def replay_scenarios():
    """name -> (state, blocks, records, (applied, height, text) wanted; height None: clean).  The honest
    chain, then one wrong block each -- wrong and properly signed, so that VerifyCommitLight of the pair
    passes and validateBlock decides -- with the text built here from the chain's own values and the
    reference's format strings (internal/state/validation.go)."""
    k, i = FAIL_AT, FAIL_AT - 1
    state, blocks, ids, records = stateful_chain()
    out = {"clean": (state, blocks, records, (N_BLOCKS - 1, None, None))}

    def wrong(name, text, header_edit=None, evidence_at=None, state_edit=None, records_edit=None, at=k, skip=0):
        st, bl, _, rec = stateful_chain(header_edit, evidence_at)
        if state_edit:
            st = dataclasses.replace(st, **state_edit)
        if records_edit:
            rec = records_edit(list(rec))
        text = text(st, bl, rec) if callable(text) else text
        out[name] = (st, bl[skip:], rec[skip:], (at - 1 - skip, at, text))

    prev_app = lambda rec: rec[i - 1].app_hash.hex().upper()  # noqa: E731
    prev_root = lambda rec: R.results_hash(as_tuples(rec[i - 1].results)).hex().upper()  # noqa: E731
    wrong("version", "wrong Block.Header.Version. Expected {11 0}, got {11 3}", _edit(version_app=3))
    wrong("version_state", "wrong Block.Header.Version. Expected {11 2}, got {11 0}", state_edit={"version_app": 2}, at=1)
    wrong("app_hash", lambda st, bl, rec: "wrong Block.Header.AppHash.  Expected %s, got %s" % (
        prev_app(rec), bl[i].header.app_hash.hex().upper()), _edit(app_hash=_flip))
    wrong("app_hash_empty", lambda st, bl, rec: "wrong Block.Header.AppHash.  Expected %s, got " % prev_app(rec),
          _edit(app_hash=b""))
    wrong("app_hash_record", lambda st, bl, rec: "wrong Block.Header.AppHash.  Expected %s, got %s" % (
        prev_app(rec), bl[i].header.app_hash.hex().upper()),
        records_edit=lambda rec: rec[:i - 1] + [dataclasses.replace(rec[i - 1], app_hash=b"\x05" * 32)] + rec[i:])
    wrong("consensus_hash", lambda st, bl, rec: "wrong Block.Header.ConsensusHash.  Expected %s, got %s" % (
        R.consensus_params_hash(22020096, -1).hex().upper(), bl[i].header.consensus_hash.hex().upper()),
        _edit(consensus_hash=_flip))
    wrong("consensus_params_state", lambda st, bl, rec: "wrong Block.Header.ConsensusHash.  Expected %s, got %s" % (
        R.consensus_params_hash(22020096, 10).hex().upper(), bl[0].header.consensus_hash.hex().upper()),
        state_edit={"block_max_gas": 10}, at=1)
    wrong("last_results_hash", lambda st, bl, rec: "wrong Block.Header.LastResultsHash.  Expected %s, got %s" % (
        prev_root(rec), bl[i].header.last_results_hash.hex().upper()), _edit(last_results_hash=_flip))

    def tamper_result(rec):
        r0 = rec[i - 1].results[0]
        rec[i - 1] = dataclasses.replace(rec[i - 1], results=[dataclasses.replace(r0, gas_used=r0.gas_used + 1)] +
                                         rec[i - 1].results[1:])
        return rec
    wrong("result_tampered", lambda st, bl, rec: "wrong Block.Header.LastResultsHash.  Expected %s, got %s" % (
        prev_root(rec), bl[i].header.last_results_hash.hex().upper()), records_edit=tamper_result)
    wrong("proposer", "block.Header.ProposerAddress %s is not a validator" % ("AB" * 20),
          _edit(proposer_address=b"\xab" * 20))
    wrong("time_equal", lambda st, bl, rec: "block time %s not greater than last block time %s" % (
        "2020-01-01 00:00:06 +0000 UTC", "2020-01-01 00:00:06 +0000 UTC"), _edit(time=(1577836806, 0)))
    wrong("time_nanos", lambda st, bl, rec: "block time %s not greater than last block time %s" % (
        "2020-01-01 00:00:05.00000012 +0000 UTC", "2020-01-01 00:00:06 +0000 UTC"), _edit(time=(1577836805, 120)))
    wrong("genesis_time", "block time 2020-01-01 00:00:01 +0000 UTC is before genesis time 2020-01-01 00:00:01.5 +0000 UTC",
          state_edit={"last_block_time": (1577836801, 500000000)}, at=1)
    wrong("below_initial_height", "block height 4 lower than initial height 50", at=4, skip=3,
          state_edit={"initial_height": 50, "last_block_height": 3, "last_block_id": ids[2],
                      "last_block_time": blocks[2].header.time, "app_hash": records[2].app_hash,
                      "last_results_hash": R.results_hash(as_tuples(records[2].results))})
    wrong("evidence_size", "Too much evidence: Max 176, got 177", evidence_at={k: EVIDENCE},
          state_edit={"evidence_max_bytes": 176})
    # two things wrong with one block: the reference's order decides
    wrong("app_hash_before_results", lambda st, bl, rec: "wrong Block.Header.AppHash.  Expected %s, got %s" % (
        prev_app(rec), bl[i].header.app_hash.hex().upper()), _edit(app_hash=_flip, last_results_hash=_flip))
    wrong("proposer_before_time", "block.Header.ProposerAddress %s is not a validator" % ("AB" * 20),
          _edit(proposer_address=b"\xab" * 20, time=(1577836806, 0)))
    wrong("results_before_evidence", lambda st, bl, rec: "wrong Block.Header.LastResultsHash.  Expected %s, got %s" % (
        prev_root(rec), bl[i].header.last_results_hash.hex().upper()), _edit(last_results_hash=_flip),
        evidence_at={k: EVIDENCE}, state_edit={"evidence_max_bytes": 10})
    # the limit itself passes (got > max fails)
    st, bl, _, rec = stateful_chain(evidence_at={k: EVIDENCE})
    out["evidence_at_limit"] = (dataclasses.replace(st, evidence_max_bytes=177), bl, rec, (N_BLOCKS - 1, None, None))
    return out


def check_replay(run, scenarios, names=None):
    """run(state, blocks, records) -> blocksync_replay_stateful's result."""
    for name, (state, blocks, records, (applied, at, text)) in scenarios.items():
        if names is not None and name not in names:
            continue
        want = (applied, None if at is None else (at, text))
        assert run(state, blocks, records) == want, name
