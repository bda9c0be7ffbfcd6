"""A chain whose validator set and consensus params change, for
chains.blocksync_replay_dynamic, with the one-block-at-a-time restatement of
the reference's loop (poolRoutine + ApplyBlock + State.Update) that the driver
must equal, shared by the CPU and GPU tests.

The generator and the restatement do the validator-set arithmetic with
tests/valset_update_ref.py and the hashes with hashlib (testing/blocks.py,
testing/factory.py), never with the host layer.

The reference's batch verifier takes keys of one type only (crypto/ed25519
Add: "pubkey is not Ed25519"), so in a set of ed25519 validators a validator of
another key type can sit in the set -- it is hashed, it can be elected -- but a
commit that carries its signature fails VerifyCommit whenever the proposer's
key type has a batch verifier.  The chain's sr25519 (or secp256k1) validator
therefore joins with little power and stays absent from the commits; the
scenario "other_key_signs" lets it sign once."""
import dataclasses
import hashlib
import random

import valset_update_ref as R
from commit_fixtures import Signer
from tendermint_amd import chains, host as H
from tendermint_amd.testing.block_wire import encode_block
from tendermint_amd.testing.blocks import (T0, commit_hash, consensus_params_hash, part_set_header, results_hash,
                                           txs_hash)
from tendermint_amd.testing.factory import _merkle, _valset_hash, header_hash
from tendermint_amd.types.canonical import (BlockID as PyBlockID, PartSetHeader, Timestamp, vote_sign_bytes,
                                            PRECOMMIT_TYPE)
from valset_update_ref import Val

CHAIN = "test_chain_id"
N_BLOCKS, N_VALS, PART_SIZE = 24, 7, 256
KINDS = {"ed25519": 0, "sr25519": 1, "secp256k1": 3}


class SecpSigner:
    def __init__(self, i: int):
        from tendermint_amd.testing.secp256k1_factory import Secp256k1Signer
        self._s = Secp256k1Signer.from_secret(b"valset chain secp %d" % i)
        self.pub_key, self.kind = self._s.public_key, 3
        self.address = R.address_of(3, self.pub_key)

    def sign(self, msg: bytes) -> bytes:
        return self._s.sign(msg)


_SIGNERS = {}


def signer(name: str):
    """name: e0, e1, ... (ed25519), s0 (sr25519), k0 (secp256k1)."""
    if name not in _SIGNERS:
        scheme = {"e": "ed25519", "s": "sr25519", "k": "secp256k1"}[name[0]]
        _SIGNERS[name] = SecpSigner(int(name[1:])) if scheme == "secp256k1" else Signer(scheme, int(name[1:]), "valset chain")
    return _SIGNERS[name]


def update(name: str, power: int) -> H.ValidatorUpdate:
    s = signer(name)
    return H.ValidatorUpdate(s.kind, s.pub_key, power)


def plan(other: str = "s0"):
    """record index -> (validator updates, consensus-param updates).  Record
    k's updates name NextValidators at block k + 1, Validators at k + 2 and
    sign LastCommit at k + 3: with 24 blocks, at windows of 1, 2, 5 and 600 a
    change of Validators falls on the first block of a window (k = 3 -> block 5
    at 5; k = 10 -> block 12 at 2) and on the last (k = 7 -> block 9 at 5 and 2;
    k = 20 -> block 22, the last one applied, at 600)."""
    return {
        1: ([update("e0", 15)], None),
        3: ([update("e7", 12)], None),
        7: ([update("e1", 0)], None),
        9: ([], chains.ConsensusParamUpdates(block=(4194304, -1))),
        10: ([update(other, 1)], None),
        13: ([update("e2", 0), update("e8", 8), update("e3", 20)], None),
        15: ([], chains.ConsensusParamUpdates(version_app=1)),
        20: ([update("e4", 11)], chains.ConsensusParamUpdates(evidence_max_bytes=2048)),
    }


def _host_set(vals, prop) -> H.ValidatorSet:
    return H.ValidatorSet([H.Validator(v.address, v.key, v.power, v.kind, v.priority) for v in vals], prop)


def _change(u: H.ValidatorUpdate) -> Val:
    return Val(R.address_of(u.key_kind, u.pub_key), u.power, 0, u.pub_key, u.key_kind)


def genesis_sets(names):
    """MakeGenesisState (internal/state/state.go): Validators = NewValidatorSet(genesis validators),
    NextValidators = its CopyIncrementProposerPriority(1), LastValidators = the empty set."""
    members = [Val(signer(n).address, 10, 0, signer(n).pub_key, signer(n).kind) for n in names]
    vals, prop = R.new_validator_set(members)
    nxt, nprop = R.increment_proposer_priority(vals, 1)
    return ([], -1), (vals, prop), (nxt, nprop)


def make_dynamic_chain(n_blocks: int = N_BLOCKS, n_vals: int = N_VALS, changes=None, seed: int = 77, header_edit=None,
                       signed_by_last=(), also_signs=None, tamper=None):
    """Heights 1..n_blocks from a genesis of n_vals ed25519 validators of power
    10; `changes` as plan() gives them.  Every header carries the real hashes of
    its state, its proposer is the state's, and block h + 1 carries the commit
    for h signed by the validators of h in set order -- those of another key type
    than ed25519 absent, unless also_signs = {height: [address]} names them.
    header_edit: {height: Header -> Header} before the header is hashed (the
    chain goes on from the edited header).  signed_by_last: heights whose commit
    the set from before (state.LastValidators) signs.  tamper: (height, index):
    one bit of that signature of the commit for `height` is flipped.
    Returns (ReplayState before block 1, [FullBlock] with raw = the block's
    protobuf bytes, [BlockID], [BlockRecord])."""
    changes = plan() if changes is None else changes
    rng = random.Random(seed)
    by_address = {}
    names = ["e%d" % i for i in range(n_vals)]
    (last, lprop), (vals, prop), (nxt, nprop) = genesis_sets(names)
    for n in list(names) + ["e7", "e8", "e9", "s0", "k0"]:
        by_address[signer(n).address] = signer(n)
    p = dict(block_max_bytes=22020096, block_max_gas=-1, evidence_max_bytes=1048576, version_app=0)
    genesis_app = bytes(rng.randrange(256) for _ in range(32))
    state = chains.ReplayState(chain_id=CHAIN, validators=_host_set(vals, prop), app_hash=genesis_app,
                               last_results_hash=results_hash([]), last_block_time=(T0, 0),
                               next_validators=_host_set(nxt, nprop), last_validators=_host_set(last, lprop),
                               pub_key_types=["ed25519", "sr25519", "secp256k1"], **p)
    blocks, ids, records = [], [], []
    last_id, last_commit = H.BlockID(), H.Commit(0, 0, H.BlockID(), [])
    app_hash, last_results = genesis_app, results_hash([])
    for h in range(1, n_blocks + 1):
        btxs = [bytes(rng.randrange(256) for _ in range(rng.randint(1, 40))) for _ in range(rng.randint(1, 3))]
        hdr = H.Header(chain_id=CHAIN, height=h, time=(T0 + h, 0), last_block_id=last_id,
                       last_commit_hash=commit_hash(last_commit), data_hash=txs_hash(btxs),
                       validators_hash=_valset_hash(_host_set(vals, prop)),
                       next_validators_hash=_valset_hash(_host_set(nxt, nprop)),
                       consensus_hash=consensus_params_hash(p["block_max_bytes"], p["block_max_gas"]),
                       app_hash=app_hash, last_results_hash=last_results, evidence_hash=_merkle([]),
                       proposer_address=vals[prop].address, version_app=p["version_app"])
        if header_edit and h in header_edit:
            hdr = header_edit[h](hdr)
        block = H.FullBlock(hdr, btxs, [], last_commit)
        block.raw = encode_block(block)[0]
        blocks.append(block)
        last_id = H.BlockID(header_hash(hdr), *part_set_header(block.raw, PART_SIZE))
        ids.append(last_id)
        # the commit for h, carried by block h + 1
        signers = last if h in signed_by_last else vals
        bid = PyBlockID(last_id.hash, PartSetHeader(last_id.psh_total, last_id.psh_hash))
        sigs = []
        for i, v in enumerate(signers):
            if v.kind != 0 and v.address not in (also_signs or {}).get(h, ()):
                sigs.append(H.CommitSig())
                continue
            ts = (T0 + h + 1, 1000 * i)
            msg = vote_sign_bytes(CHAIN, PRECOMMIT_TYPE, h, 0, bid, Timestamp(*ts))
            sig = by_address[v.address].sign(msg)
            if tamper == (h, i):
                sig = bytes([sig[0] ^ 1]) + sig[1:]
            sigs.append(H.CommitSig(H.BLOCK_ID_FLAG_COMMIT, v.address, ts, sig))
        last_commit = H.Commit(h, 0, last_id, sigs)
        # the application's answer and State.Update
        results = [H.TxResult(rng.choice([0, 0, 1]), bytes(rng.randrange(256) for _ in range(rng.randint(0, 20))),
                              rng.choice([0, 1000]), rng.choice([0, 999])) for _ in btxs]
        ups, pu = changes.get(h - 1, ([], None))
        rec = chains.BlockRecord(results, bytes(rng.randrange(256) for _ in range(32)), list(ups), pu)
        records.append(rec)
        app_hash, last_results = rec.app_hash, results_hash(results)
        new = R.update_with_change_set(nxt, [_change(u) for u in ups]) if ups else nxt
        new, newprop = R.increment_proposer_priority(new, 1)
        (last, lprop), (vals, prop), (nxt, nprop) = (vals, prop), (nxt, nprop), (new, newprop)
        if pu is not None:
            if pu.block is not None:
                p["block_max_bytes"], p["block_max_gas"] = pu.block
            if pu.evidence_max_bytes is not None:
                p["evidence_max_bytes"] = pu.evidence_max_bytes
            if pu.version_app is not None:
                p["version_app"] = pu.version_app
    return state, blocks, ids, records


# ---- the one-block-at-a-time restatement ----
def _ref(vs: H.ValidatorSet):
    return [Val(v.address, v.voting_power, v.proposer_priority, v.pub_key, v.key_kind) for v in vs.validators]


def _upd_str(u):
    return "{%s:%s %d}" % ({0: "ed25519", 1: "sr25519", 3: "secp256k1"}.get(u.key_kind, "kind%d" % u.key_kind),
                           u.pub_key.hex().upper(), u.power)


def _validate_params(p):
    if p["block_max_bytes"] <= 0:
        return "block.MaxBytes must be greater than 0. Got %d" % p["block_max_bytes"]
    if p["block_max_bytes"] > 104857600:
        return "block.MaxBytes is too big. %d > %d" % (p["block_max_bytes"], 104857600)
    if p["block_max_gas"] < -1:
        return "block.MaxGas must be greater or equal to -1. Got %d" % p["block_max_gas"]
    if p["evidence_max_bytes"] > p["block_max_bytes"]:
        return "evidence.MaxBytesEvidence is greater than upper bound, %d > %d" % (p["evidence_max_bytes"],
                                                                                  p["block_max_bytes"])
    if p["evidence_max_bytes"] < 0:
        return "evidence.MaxBytes must be non negative. Got: %d" % p["evidence_max_bytes"]
    if not p["pub_key_types"]:
        return "len(Validator.PubKeyTypes) must be greater than 0"
    for i, t in enumerate(p["pub_key_types"]):
        if t not in KINDS:
            return "params.Validator.PubKeyTypes[%d], %s, is an unknown pubkey type" % (i, t)
    return None


def replay_one_at_a_time(backend, state, blocks, records):
    """poolRoutine's loop, one pair at a time: VerifyCommitLight of the pair,
    validateBlock against the state, then ApplyBlock's validateValidatorUpdates
    and State.Update.  backend: verify_commit / verify_commit_light of one
    commit (tests/commit_fixtures.py).  Block.ValidateBasic is not restated: the
    chains here pass it.  Returns (applied, (height, text) or None, the state
    after as a dict)."""
    hx = lambda b: b.hex().upper()  # noqa: E731
    st = dict(last=state.last_validators or state.validators, vals=state.validators,
              next=state.next_validators or state.validators, last_block_id=state.last_block_id or H.BlockID(),
              last_block_height=state.last_block_height, last_block_time=tuple(state.last_block_time),
              app_hash=state.app_hash, last_results_hash=state.last_results_hash,
              vals_changed=state.last_height_validators_changed,
              params_changed=state.last_height_consensus_params_changed,
              params=dict(block_max_bytes=state.block_max_bytes, block_max_gas=state.block_max_gas,
                          evidence_max_bytes=state.evidence_max_bytes, version_app=state.version_app,
                          pub_key_types=list(state.pub_key_types)))
    applied = 0
    for g in range(len(blocks) - 1):
        first, second, hd, p = blocks[g], blocks[g + 1], blocks[g].header, st["params"]
        first_id = H.BlockID(header_hash(hd), *part_set_header(first.raw, PART_SIZE))
        err = backend.verify_commit_light(CHAIN, st["vals"], first_id, hd.height, second.last_commit)

        def check():
            if (hd.version_block, hd.version_app) != (state.version_block, p["version_app"]):
                return "wrong Block.Header.Version. Expected {%d %d}, got {%d %d}" % (
                    state.version_block, p["version_app"], hd.version_block, hd.version_app)
            if hd.chain_id != CHAIN:
                return "wrong Block.Header.ChainID. Expected %s, got %s" % (CHAIN, hd.chain_id)
            if st["last_block_height"] == 0 and hd.height != state.initial_height:
                return "wrong Block.Header.Height. Expected %d for initial block, got %d" % (hd.height, state.initial_height)
            if st["last_block_height"] > 0 and hd.height != st["last_block_height"] + 1:
                return "wrong Block.Header.Height. Expected %d, got %d" % (st["last_block_height"] + 1, hd.height)
            if not hd.last_block_id.equals(st["last_block_id"]):
                return "wrong Block.Header.LastBlockID.  Expected %s, got %s" % (
                    chains._block_id_string(st["last_block_id"]), chains._block_id_string(hd.last_block_id))
            for name, want, got in (
                    ("AppHash", st["app_hash"], hd.app_hash),
                    ("ConsensusHash", consensus_params_hash(p["block_max_bytes"], p["block_max_gas"]), hd.consensus_hash),
                    ("LastResultsHash", st["last_results_hash"], hd.last_results_hash),
                    ("ValidatorsHash", _valset_hash(st["vals"]), hd.validators_hash),
                    ("NextValidatorsHash", _valset_hash(st["next"]), hd.next_validators_hash)):
                if want != got:
                    return "wrong Block.Header.%s.  Expected %s, got %s" % (name, hx(want), hx(got))
            if hd.height == state.initial_height:
                if first.last_commit.signatures:
                    return "initial block can't have LastCommit signatures"
            else:
                e = backend.verify_commit(CHAIN, st["last"], st["last_block_id"], hd.height - 1, first.last_commit)
                if e is not None:
                    return e
            if hd.proposer_address not in {v.address for v in st["vals"].validators}:
                return "block.Header.ProposerAddress %s is not a validator" % hx(hd.proposer_address)
            if hd.height > state.initial_height and not tuple(hd.time) > st["last_block_time"]:
                return "block time %s not greater than last block time %s" % (
                    chains.go_time_string(hd.time), chains.go_time_string(st["last_block_time"]))
            if hd.height == state.initial_height and tuple(hd.time) < st["last_block_time"]:
                return "block time %s is before genesis time %s" % (chains.go_time_string(hd.time),
                                                                    chains.go_time_string(st["last_block_time"]))
            got = chains.evidence_byte_size(first.evidence)
            if got > p["evidence_max_bytes"]:
                return "Too much evidence: Max %d, got %d" % (p["evidence_max_bytes"], got)
            # ApplyBlock: validateValidatorUpdates, PB2TM.ValidatorUpdates
            rec = records[g]
            ups = [u if isinstance(u, H.ValidatorUpdate) else H.ValidatorUpdate(*u) for u in rec.validator_updates]
            sizes = {0: ("PubKeyEd25519", 32), 1: ("PubKeySr25519", 32), 3: ("PubKeySecp256k1", 33)}

            def key_error(u):
                if u.key_kind not in sizes:
                    return "fromproto: key type %d is not supported" % u.key_kind
                if len(u.pub_key) != sizes[u.key_kind][1]:
                    return "invalid size for %s. Got %d, expected %d" % (sizes[u.key_kind][0], len(u.pub_key),
                                                                         sizes[u.key_kind][1])
            for u in ups:
                if u.power < 0:
                    return "error in validator updates: voting power can't be negative %s" % _upd_str(u)
                if u.power == 0:
                    continue
                if key_error(u):
                    return "error in validator updates: " + key_error(u)
                name = {0: "ed25519", 1: "sr25519", 3: "secp256k1"}[u.key_kind]
                if name not in p["pub_key_types"]:
                    return "error in validator updates: validator %s is using pubkey %s, which is unsupported for " \
                           "consensus" % (_upd_str(u), name)
            for u in ups:
                if key_error(u):
                    return key_error(u)
            # State.Update
            nxt, vals_changed = _ref(st["next"]), st["vals_changed"]
            if ups:
                try:
                    nxt = R.update_with_change_set(nxt, [_change(u) for u in ups])
                except R.ValsetError as e:
                    return "commit failed for application: changing validator set: %s" % e
                vals_changed = hd.height + 2
            nxt, nprop = R.increment_proposer_priority(nxt, 1)
            np_, params_changed = p, st["params_changed"]
            pu = rec.consensus_param_updates
            if pu is not None:
                np_ = dict(p)
                if pu.block is not None:
                    np_["block_max_bytes"], np_["block_max_gas"] = pu.block
                if pu.evidence_max_bytes is not None:
                    np_["evidence_max_bytes"] = pu.evidence_max_bytes
                if pu.pub_key_types is not None:
                    np_["pub_key_types"] = list(pu.pub_key_types)
                if pu.version_app is not None:
                    np_["version_app"] = pu.version_app
                e = _validate_params(np_)
                if e is not None:
                    return "commit failed for application: updating consensus params: " + e
                params_changed = hd.height + 1
            st.update(last=st["vals"], vals=st["next"], next=_host_set(nxt, nprop), last_block_id=first_id,
                      last_block_height=hd.height, last_block_time=tuple(hd.time), app_hash=rec.app_hash,
                      last_results_hash=results_hash(rec.results), vals_changed=vals_changed,
                      params_changed=params_changed, params=np_)
            return None
        err = err or check()
        if err is not None:
            return applied, (hd.height, err), st
        applied += 1
    return applied, None, st


def state_dict(s: chains.ReplayState):
    """A ReplayState in the restatement's terms."""
    return dict(last=s.last_validators, vals=s.validators, next=s.next_validators, last_block_id=s.last_block_id,
                last_block_height=s.last_block_height, last_block_time=tuple(s.last_block_time), app_hash=s.app_hash,
                last_results_hash=s.last_results_hash, vals_changed=s.last_height_validators_changed,
                params_changed=s.last_height_consensus_params_changed,
                params=dict(block_max_bytes=s.block_max_bytes, block_max_gas=s.block_max_gas,
                            evidence_max_bytes=s.evidence_max_bytes, version_app=s.version_app,
                            pub_key_types=list(s.pub_key_types)))


def same_state(a, b) -> bool:
    """Two state dicts; the sets by members, priorities and proposer."""
    sets = lambda d: [([dataclasses.astuple(v) for v in d[k].validators],  # noqa: E731
                       d[k].validators[d[k].proposer_index].address if d[k].validators else None)
                      for k in ("last", "vals", "next")]
    rest = lambda d: {k: v for k, v in d.items() if k not in ("last", "vals", "next")}  # noqa: E731
    return sets(a) == sets(b) and rest(a) == rest(b)


# ---- the scenarios: one cause each, in a chain that is valid otherwise ----
def _replace(records, g, **kw):
    out = list(records)
    out[g] = dataclasses.replace(out[g], **kw)
    return out


def scenarios(other: str = "s0"):
    """name -> (state, blocks, records): the honest chain, then one wrong thing
    each.  The texts come from the restatement."""
    pl = plan(other)
    honest = make_dynamic_chain(changes=pl)
    state, blocks, ids, records = honest
    out = {"clean": (state, blocks, records)}
    stale_vals = blocks[4].header.validators_hash      # block index 5 (height 6) is the first under e7's set
    stale_next = blocks[3].header.next_validators_hash  # block index 4 (height 5) is the first to name it
    removed = signer("e1").address                     # out of Validators from block index 9 (height 10)

    def edited(name, height, **kw):
        st, bl, _, rec = make_dynamic_chain(changes=pl, header_edit={height: lambda h: dataclasses.replace(h, **kw)})
        out[name] = (st, bl, rec)
    edited("stale_validators_hash", 6, validators_hash=stale_vals)
    edited("stale_next_validators_hash", 5, next_validators_hash=stale_next)
    edited("removed_proposer", 11, proposer_address=removed)
    st, bl, _, rec = make_dynamic_chain(changes=pl, signed_by_last=(6,))  # height 6 is the first under e7's set
    out["signed_by_the_old_set"] = (st, bl, rec)
    other_address = signer(other).address
    st, bl, _, rec = make_dynamic_chain(changes=pl, also_signs={14: [other_address]})
    out["other_key_signs"] = (st, bl, rec)
    st, bl, _, rec = make_dynamic_chain(changes=pl, tamper=(7, 2))
    out["tampered_signature"] = (st, bl, rec)
    bad = {
        "negative_power": dict(validator_updates=[update("e5", -3)]),
        "unsupported_key_type": dict(validator_updates=[update("k0", 5)]),
        "unknown_removal": dict(validator_updates=[update("e9", 0)]),
        "emptying_the_set": dict(validator_updates=[H.ValidatorUpdate(v.key_kind, v.pub_key, 0)
                                                    for v in state.validators.validators]),
        "duplicate_update": dict(validator_updates=[update("e5", 4), update("e5", 6)]),
        "short_key": dict(validator_updates=[H.ValidatorUpdate(0, b"\x01" * 31, 5)]),
        "block_max_bytes_zero": dict(consensus_param_updates=chains.ConsensusParamUpdates(block=(0, -1))),
        "evidence_above_block": dict(consensus_param_updates=chains.ConsensusParamUpdates(evidence_max_bytes=22020097)),
        "max_gas_below": dict(consensus_param_updates=chains.ConsensusParamUpdates(block=(1024 * 1024, -2))),
        "no_key_types": dict(consensus_param_updates=chains.ConsensusParamUpdates(pub_key_types=[])),
        "unknown_key_type": dict(consensus_param_updates=chains.ConsensusParamUpdates(pub_key_types=["ed25519", "bls"])),
    }
    for name, kw in bad.items():
        out[name] = (state, blocks, _replace(records, 2, **kw))
    # the validator set fails before the params of the same block do
    out["set_before_params"] = (state, blocks, _replace(
        records, 2, validator_updates=[update("e9", 0)],
        consensus_param_updates=chains.ConsensusParamUpdates(block=(0, -1))))
    st2 = dataclasses.replace(state, pub_key_types=["ed25519", "sr25519"])
    out["unsupported_key_type"] = (st2, blocks, _replace(records, 2, validator_updates=[update("k0", 5)]))
    return out
