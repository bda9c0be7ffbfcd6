"""A consistent chain of host.FullBlock for blocksync's full validation
(chains.blocksync_replay_full): unlike factory.make_block_chain, whose headers
carry random hashes, every header here has the real LastCommitHash, DataHash
and EvidenceHash of its block, its LastBlockID is the previous block's
BlockID{Header.Hash, part-set header of `raw`}, and every commit signs that
BlockID.  `raw` is arbitrary bytes of a chosen length (only its part set is read),
or with wire=True the block's real protobuf encoding (testing/block_wire.py),
so that the BlockIDs and signatures bind to the part sets of real blocks
(chains.blocksync_replay_wire).  make_stateful_chain adds a recorded
application: the headers then carry the real AppHash, ConsensusHash and
LastResultsHash as well (chains.blocksync_replay_stateful).  Input generation
only; the hashes are restated with hashlib, never taken from the engine.
"""
from __future__ import annotations

import hashlib
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .block_wire import encode_block
from .factory import _field, _merkle, _uvarint, _valset_hash, header_hash, key_seed

T0 = 1577836800


def commit_sig_bytes(s) -> bytes:
    """tmproto.CommitSig.Marshal (proto/tendermint/types/types.pb.go:1764-1797)
    of a host.CommitSig."""
    secs, nanos = s.timestamp
    ts = (b"\x08" + _uvarint(secs) if secs else b"") + (b"\x10" + _uvarint(nanos) if nanos else b"")
    return ((b"\x08" + _uvarint(s.block_id_flag) if s.block_id_flag else b"") +
            (_field(0x12, s.validator_address) if s.validator_address else b"") + _field(0x1A, ts) +
            (_field(0x22, s.signature) if s.signature else b""))


def commit_hash(c) -> bytes:
    """Commit.Hash (types/block.go:900-918)."""
    return _merkle([commit_sig_bytes(s) for s in c.signatures])


def txs_hash(txs: Sequence[bytes]) -> bytes:
    """Txs.Hash (types/tx.go:34-39)."""
    return _merkle([hashlib.sha256(t).digest() for t in txs])


def part_set_header(raw: bytes, part_size: int) -> Tuple[int, bytes]:
    """NewPartSetFromData(raw, part_size).Header() (types/part_set.go:172-222)."""
    parts = [raw[i:i + part_size] for i in range(0, len(raw), part_size)]
    return len(parts), _merkle(parts)


def tx_result_bytes(r) -> bytes:
    """ExecTxResult.Marshal of a host.TxResult's deterministic fields
    (abci/types/types.go:213-222, types.pb.go:3165-3170)."""
    return ((b"\x08" + _uvarint(r.code) if r.code else b"") + (_field(0x12, r.data) if r.data else b"") +
            (b"\x28" + _uvarint(r.gas_wanted) if r.gas_wanted else b"") +
            (b"\x30" + _uvarint(r.gas_used) if r.gas_used else b""))


def results_hash(results, first: Optional[bytes] = None) -> bytes:
    """The merkle root over abci.MarshalTxResults: State.LastResultsHash
    (internal/state/execution.go:262-267); with `first`, the light client's
    form with its leading leaf (light/rpc/client.go:452-464)."""
    return _merkle(([first] if first is not None else []) + [tx_result_bytes(r) for r in results])


def consensus_params_hash(block_max_bytes: int, block_max_gas: int) -> bytes:
    """ConsensusParams.HashConsensusParams (types/params.go:385-399)."""
    return hashlib.sha256((b"\x08" + _uvarint(block_max_bytes) if block_max_bytes else b"") +
                          (b"\x10" + _uvarint(block_max_gas) if block_max_gas else b"")).digest()


class _Execution:
    """A recorded application for make_stateful_chain: one result per
    transaction and an app hash per block, drawn from a generator of its own
    (make_full_chain's draws stay as they are)."""

    def __init__(self, seed: int, data_len: Sequence[int], block_max_bytes: int, block_max_gas: int):
        from .. import chains
        self.rng = random.Random(seed * 7919 + 1)
        self.data_len = data_len
        self.consensus_hash = consensus_params_hash(block_max_bytes, block_max_gas)
        self.genesis_app_hash = bytes(self.rng.randrange(256) for _ in range(32))
        self.records: List = []
        self._record = chains.BlockRecord

    def before(self, h: int) -> Tuple[bytes, bytes]:
        """(AppHash, LastResultsHash) of the state that block h is validated against."""
        if not self.records:
            return self.genesis_app_hash, results_hash([])
        return self.records[-1].app_hash, results_hash(self.records[-1].results)

    def execute(self, btxs) -> None:
        from .. import host as H
        rng = self.rng
        results = [H.TxResult(rng.choice([0, 0, 0, 1, 14, 1 << 31]), bytes(rng.randrange(256) for _ in range(
            rng.randint(*self.data_len))), rng.choice([0, 1000, 200000, -1]), rng.choice([0, 999, 65536]))
            for _ in btxs]
        self.records.append(self._record(results, bytes(rng.randrange(256) for _ in range(32))))


def make_stateful_chain(n_blocks: int, n_vals: int = 5, chain_id: str = "test_chain_id", seed: int = 23,
                        data_len: Sequence[int] = (0, 40), block_max_bytes: int = 22020096, block_max_gas: int = -1,
                        evidence_max_bytes: int = 1048576, **kw):
    """make_full_chain whose headers also carry the real AppHash,
    ConsensusHash and LastResultsHash of a recorded application: block h's
    record holds one result per transaction (data of data_len[0]..data_len[1]
    bytes) and a random app hash, and block h + 1's header commits to both.
    Returns (ReplayState before block 1, [FullBlock], [BlockID], [BlockRecord]);
    **kw goes to make_full_chain (wire=True among them)."""
    from .. import chains
    ex = _Execution(seed, data_len, block_max_bytes, block_max_gas)
    vals, blocks, ids = make_full_chain(n_blocks, n_vals, chain_id, seed, _execution=ex, **kw)
    state = chains.ReplayState(chain_id=chain_id, validators=vals, app_hash=ex.genesis_app_hash,
                               last_results_hash=results_hash([]), last_block_time=(T0, 0),
                               block_max_bytes=block_max_bytes, block_max_gas=block_max_gas,
                               evidence_max_bytes=evidence_max_bytes)
    return state, blocks, ids, ex.records


def make_full_chain(n_blocks: int, n_vals: int = 5, chain_id: str = "test_chain_id", seed: int = 23,
                    raw_len: Sequence[int] = (1, 70000), part_size: int = 65536, txs: Sequence[int] = (0, 5),
                    tx_len: Sequence[int] = (1, 300), evidence_at: Optional[dict] = None,
                    absent: Sequence[int] = (), sign: bool = True, header_edit: Optional[dict] = None,
                    _execution: Optional[_Execution] = None, wire: bool = False):
    """Heights 1..n_blocks (initial height 1) over a static n_vals-validator set
    of power 10.  Block h carries LastCommit = the commit for h-1 (a commit
    without signatures at height 1), txs[0]..txs[1] transactions of
    tx_len[0]..tx_len[1] bytes, evidence_at.get(h, []) as its evidence list
    and raw_len[0]..raw_len[1] bytes of `raw`.  The validators whose index is
    in `absent` do not sign (BlockIDFlagAbsent entries).  sign=False fills the
    signatures with random bytes (hashing benchmarks: nothing verifies them).
    header_edit: {height: function Header -> Header} applied before the header
    is hashed, so the chain goes on from the edited header and its commit signs
    it (a block that is wrong and properly signed).
    wire=True sets each block's `raw` to its canonical protobuf encoding
    (block_wire.encode_block) in place of the drawn bytes; the draws themselves
    stay the same, so the transactions and keys do not depend on the switch.
    Returns (ValidatorSet, [FullBlock], [BlockID of each block])."""
    from .. import host as H
    from ..types.canonical import BlockID, PartSetHeader
    from . import bulk
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    seeds = [key_seed(i, "fkey") for i in range(n_vals)]
    pks = bulk.public_keys(seeds)
    addr = [hashlib.sha256(pk).digest()[:20] for pk in pks]
    ks = sorted(range(n_vals), key=lambda k: addr[k])
    vals = H.ValidatorSet([H.Validator(addr[k], pks[k], 10) for k in ks], proposer_index=0)
    vh = _valset_hash(vals)
    signing = [i for i in range(n_vals) if i not in set(absent)]
    evidence_at = evidence_at or {}
    consensus_hash, app_hash, results_hash = (bytes(rng.randrange(256) for _ in range(32)) for _ in range(3))
    blocks: List[H.FullBlock] = []
    ids: List[H.BlockID] = []
    last_id = H.BlockID()
    last_commit = H.Commit(0, 0, H.BlockID(), [])
    for h in range(1, n_blocks + 1):
        btxs = [nrng.bytes(rng.randint(*tx_len)) for _ in range(rng.randint(*txs))]
        evs = list(evidence_at.get(h, []))
        raw = nrng.bytes(rng.randint(*raw_len))
        if _execution is not None:  # the state block h is validated against, then h's own record
            consensus_hash = _execution.consensus_hash
            app_hash, results_hash = _execution.before(h)
            _execution.execute(btxs)
        hdr = H.Header(chain_id=chain_id, height=h, time=(T0 + h, 0), last_block_id=last_id,
                       last_commit_hash=commit_hash(last_commit), data_hash=txs_hash(btxs), validators_hash=vh,
                       next_validators_hash=vh, consensus_hash=consensus_hash, app_hash=app_hash,
                       last_results_hash=results_hash, evidence_hash=_merkle(evs),
                       proposer_address=vals.validators[0].address)
        if header_edit and h in header_edit:
            hdr = header_edit[h](hdr)
        if wire:
            raw = encode_block(H.FullBlock(hdr, btxs, evs, last_commit))[0]
        blocks.append(H.FullBlock(hdr, btxs, evs, last_commit, raw))
        total, phash = part_set_header(raw, part_size)
        last_id = H.BlockID(header_hash(hdr), total, phash)
        ids.append(last_id)
        # the commit for height h, carried by block h + 1
        secs, nanos = [T0 + h + 1] * len(signing), [1000 * i for i in signing]
        if sign:
            bid = BlockID(last_id.hash, PartSetHeader(last_id.psh_total, last_id.psh_hash))
            msg, off = bulk.vote_messages(bulk.commit_vote_head(h, 0, bid), chain_id, secs, nanos)
            raw_sigs = bulk.sign_many(seeds, np.asarray([ks[i] for i in signing], np.uint32), msg, off).tobytes()
        else:
            raw_sigs = nrng.bytes(64 * len(signing))
        by_index = {i: H.CommitSig(H.BLOCK_ID_FLAG_COMMIT, vals.validators[i].address, (secs[k], nanos[k]),
                                   raw_sigs[64 * k:64 * k + 64]) for k, i in enumerate(signing)}
        last_commit = H.Commit(h, 0, last_id, [by_index.get(i, H.CommitSig()) for i in range(n_vals)])
    return vals, blocks, ids
