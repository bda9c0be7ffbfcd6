"""Consensus per-vote batching (ADR-064,
docs/architecture/adr-064-batch-verification.md:58-64): the reference's
VoteSet (types/vote_set.go) with its signature checks moved into batches.

  * VoteSet.add_vote(vote)   == VoteSet.AddVote (types/vote_set.go:150-245),
                                one vote, one signature check
  * VoteSet.add_votes(votes) == AddVote of each vote in order, with the
                                signature checks of all of them in ONE engine
                                call (tmv_verify_vote_batch)
  * VoteBuffer               the ADR's consensus flow: votes are held until
                                the pending ones carry more than 2/3 of the
                                voting power, verified together, then later
                                votes are verified as they arrive

  * VoteSet(..., extensions_enabled=True)
                             == NewExtendedVoteSet (types/vote_set.go:95-103):
                                every vote goes through VerifyVoteAndExtension
                                (types/vote.go:245-262), so a non-nil precommit
                                carries TWO signatures of its validator, the
                                second over VoteExtensionSignBytes; both go
                                into the same engine call
                                (tmv_verify_extended_votes)
  * extended_commits_to_vote_sets(jobs)
                             == ExtendedCommit.ToExtendedVoteSet
                                (types/block.go:1037-1071) under
                                votesFromExtendedCommit
                                (internal/consensus/state.go:722-732) for many
                                extended commits, the 2n signatures of all of
                                them in one engine call

Bookkeeping (votes by validator, votes by block, the first 2/3 majority,
conflicting votes) follows vote_set.go:247-314 (addVerifiedVote) and
:685-692 (blockVotes).  Error texts are the reference's.  Peer 2/3 claims
(SetPeerMaj23), MakeCommit / MakeExtendedCommit and the ABCI
VerifyVoteExtension call into the application are out of scope.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

from . import host as H
from .host import Vote

_TYPE_NAME = {H.PREVOTE_TYPE: "Prevote", H.PRECOMMIT_TYPE: "Precommit"}


def _hexu(b: bytes) -> str:
    return b.hex().upper()


def _fp(b: bytes) -> str:  # %X of libs/bytes.Fingerprint (first 6 bytes, zero padded)
    return _hexu((b + b"\0" * 6)[:6])


def _canonical_time(ts: Tuple[int, int]) -> str:
    import datetime
    secs, nanos = ts
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=secs)
    frac = ("%09d" % nanos).rstrip("0")
    return t.strftime("%Y-%m-%dT%H:%M:%S") + ("." + frac if frac else "") + "Z"


def vote_string(v: Vote) -> str:
    """Vote.String() (types/vote.go:191-224)."""
    bh = _fp(v.block_id.hash) if v.block_id.hash else "nil"
    return "Vote{%d:%s %d/%d %s %s %s %d @ %s}" % (v.validator_index, _fp(v.validator_address), v.height, v.round,
                                                  _TYPE_NAME.get(v.type, "?"), bh, _fp(v.signature), len(v.extension),
                                                  _canonical_time(v.timestamp))


def _block_key(b: H.BlockID):
    return (b.hash, b.psh_total, b.psh_hash)


def _pubkey_string(kind: int, pk: bytes) -> str:
    name = {H.TMV_KIND_ED25519: "PubKeyEd25519{%s}", H.TMV_KIND_SECP256K1: "PubKeySecp256k1{%s}"}
    return name.get(kind, "PubKeySr25519{%s}") % _hexu(pk)


VerifyFn = Callable[[str, List[Vote], List[Tuple[int, bytes]]], List[int]]


class VoteSet:
    """types.VoteSet for one (height, round, type), verifying signatures
    through `verify` (list of votes + their validators' keys -> TMV_VOTE_*
    per vote; e.g. lambda c, v, k: host.verify_vote_batch(ctx, c, v, k))."""

    def __init__(self, chain_id: str, height: int, round_: int, msg_type: int, vals: H.ValidatorSet,
                 verify: Optional[VerifyFn], extensions_enabled: bool = False,
                 verify_extended: Optional[VerifyFn] = None):
        """extensions_enabled: NewExtendedVoteSet; the signatures are then
        checked by `verify_extended` (same arguments and results as `verify`,
        with VerifyVoteAndExtension's meaning; e.g. lambda c, v, k: [r for r, _
        in host.verify_extended_votes(ctx, host.VOTE_MODE_VERIFY_AND_EXTENSION,
        c, v, k)]) and `verify` is not used."""
        self.chain_id, self.height, self.round, self.type, self.vals = chain_id, height, round_, msg_type, vals
        self.verify = verify
        self.extensions_enabled = extensions_enabled
        self.verify_extended = verify_extended
        if extensions_enabled and verify_extended is None:
            raise ValueError("an extended vote set needs verify_extended")
        n = len(vals.validators)
        self.votes: List[Optional[Vote]] = [None] * n
        self.sum = 0
        self.maj23: Optional[H.BlockID] = None
        self.votes_by_block: Dict[tuple, dict] = {}
        self.signature_batches = 0  # engine calls made (tests / metrics)

    # -------------------------------------------------------------- reference API
    def total_power(self) -> int:
        return self.vals.total_voting_power()

    def has_two_thirds_majority(self) -> bool:
        return self.maj23 is not None

    def two_thirds_majority(self) -> Tuple[Optional[H.BlockID], bool]:
        return (self.maj23, True) if self.maj23 is not None else (H.BlockID(), False)

    def has_two_thirds_any(self) -> bool:
        return self.sum > self.total_power() * 2 // 3

    def get_by_index(self, i: int) -> Optional[Vote]:
        return self.votes[i] if 0 <= i < len(self.votes) else None

    def add_vote(self, vote: Optional[Vote]) -> Tuple[bool, Optional[str]]:
        return self.add_votes([vote])[0]

    def add_votes(self, votes: List[Optional[Vote]]) -> List[Tuple[bool, Optional[str]]]:
        """AddVote of each vote in order; the signatures of every vote that
        passes the pre-signature checks are verified in one batch first."""
        pre = [self._precheck(v) for v in votes]
        cand = [i for i, p in enumerate(pre) if p is None]
        sig_res: Dict[int, int] = {}
        if cand:
            keys = [(self.vals.validators[votes[i].validator_index].key_kind,
                     self.vals.validators[votes[i].validator_index].pub_key) for i in cand]
            check = self.verify_extended if self.extensions_enabled else self.verify
            res = check(self.chain_id, [votes[i] for i in cand], keys)
            self.signature_batches += 1
            sig_res = dict(zip(cand, res))
        out = []
        for i, v in enumerate(votes):
            if pre[i] is not None:
                out.append(pre[i])
                continue
            out.append(self._add_checked(v, sig_res[i]))
        return out

    # -------------------------------------------------------------- internals
    def _precheck(self, vote: Optional[Vote]) -> Optional[Tuple[bool, Optional[str]]]:
        """types/vote_set.go:163-199: everything addVote checks before the
        signature; None = go on to the signature."""
        if vote is None:
            return False, "nil vote"
        if vote.validator_index < 0:
            return False, "index < 0: invalid validator index"
        if not vote.validator_address:
            return False, "empty address: invalid validator address"
        if (vote.height, vote.round, vote.type) != (self.height, self.round, self.type):
            return False, ("expected %d/%d/%d, but got %d/%d/%d: unexpected step" %
                           (self.height, self.round, self.type, vote.height, vote.round, vote.type))
        if vote.validator_index >= len(self.vals.validators):
            return False, ("cannot find validator %d in valSet of size %d: invalid validator index" %
                           (vote.validator_index, len(self.vals.validators)))
        val = self.vals.validators[vote.validator_index]
        if vote.validator_address != val.address:
            return False, ("vote.ValidatorAddress (%s) does not match address (%s) for vote.ValidatorIndex (%d)\n"
                           "Ensure the genesis file is correct across all validators: invalid validator address" %
                           (_hexu(vote.validator_address), _hexu(val.address), vote.validator_index))
        return None

    def _get_vote(self, idx: int, key: tuple) -> Optional[Vote]:
        ex = self.votes[idx]
        if ex is not None and _block_key(ex.block_id) == key:
            return ex
        bv = self.votes_by_block.get(key)
        return bv["votes"].get(idx) if bv else None

    def _add_checked(self, vote: Vote, sig: int) -> Tuple[bool, Optional[str]]:
        """types/vote_set.go:201-245 from the duplicate check on, with the
        signature result already known."""
        # duplicate / non-deterministic signature checks precede the
        # signature check in the reference: re-run the pre-checks' state-
        # dependent part now, against votes added earlier in this batch
        key = _block_key(vote.block_id)
        ex = self._get_vote(vote.validator_index, key)
        if ex is not None:
            if ex.signature == vote.signature:
                return False, None
            return False, "existing vote: %s; new vote: %s: non-deterministic signature" % (vote_string(ex),
                                                                                          vote_string(vote))
        if sig != H.VOTE_OK:
            val = self.vals.validators[vote.validator_index]
            why = "invalid validator address" if sig == H.VOTE_ERR_INVALID_ADDRESS else "invalid signature"
            return False, "failed to verify vote with ChainID %s and PubKey %s: %s" % (
                self.chain_id, _pubkey_string(val.key_kind, val.pub_key), why)
        if not self.extensions_enabled and (vote.extension_signature or vote.extension):  # vote_set.go:218-220
            return False, "unexpected vote extension data present in vote"
        added, conflicting = self._add_verified(vote, key, self.vals.validators[vote.validator_index].voting_power)
        if conflicting is not None:
            return added, "conflicting votes from validator %s" % _hexu(conflicting.validator_address)
        return added, None

    def _add_verified(self, vote: Vote, key: tuple, power: int):
        """types/vote_set.go:247-314."""
        idx = vote.validator_index
        conflicting = None
        ex = self.votes[idx]
        if ex is not None:
            conflicting = ex
            if self.maj23 is not None and _block_key(self.maj23) == key:
                self.votes[idx] = vote
        else:
            self.votes[idx] = vote
            self.sum += power
        bv = self.votes_by_block.get(key)
        if bv is not None:
            if conflicting is not None and not bv["peer_maj23"]:
                return False, conflicting
        else:
            if conflicting is not None:
                return False, conflicting
            bv = {"peer_maj23": False, "votes": {}, "sum": 0}
            self.votes_by_block[key] = bv
        orig = bv["sum"]
        quorum = self.total_power() * 2 // 3 + 1
        if idx not in bv["votes"]:  # blockVotes.addVerifiedVote (:685-692)
            bv["votes"][idx] = vote
            bv["sum"] += power
        if orig < quorum <= bv["sum"] and self.maj23 is None:
            self.maj23 = vote.block_id
            for i, v in bv["votes"].items():
                self.votes[i] = v
        return True, conflicting


class VoteBuffer:
    """ADR-064's consensus flow over a VoteSet: votes are held until the
    pending ones carry more than 2/3 of the voting power, then verified and
    added in one batch (add_votes); after that each vote goes straight in.
    Results come back per vote in arrival order as they are decided."""

    def __init__(self, vote_set: VoteSet):
        self.vs = vote_set
        self.pending: List[Vote] = []
        self.pending_power = 0
        self.flushed = False

    def add(self, vote: Vote) -> List[Tuple[Vote, Tuple[bool, Optional[str]]]]:
        if self.flushed:
            return [(vote, self.vs.add_vote(vote))]
        self.pending.append(vote)
        val = self.vs.vals.validators[vote.validator_index] \
            if 0 <= vote.validator_index < len(self.vs.vals.validators) else None
        if val is not None:
            self.pending_power += val.voting_power
        if self.pending_power > self.vs.total_power() * 2 // 3:
            return self.flush()
        return []

    def flush(self) -> List[Tuple[Vote, Tuple[bool, Optional[str]]]]:
        votes, self.pending, self.pending_power = self.pending, [], 0
        self.flushed = True
        return list(zip(votes, self.vs.add_votes(votes)))


# ---------------------------------------------------------------- vote extensions: restatements
MAX_SIGNATURE_SIZE = 64                # types/vote.go: max(ed25519.SignatureSize, 64)
MAX_VOTE_EXTENSION_SIZE = 1024 * 1024  # types/vote.go:20


def _block_id_is_nil(b: H.BlockID) -> bool:
    return not b.hash and b.psh_total == 0 and not b.psh_hash


def _block_id_string(b: H.BlockID) -> str:  # BlockID.String (types/block.go:1416-1418)
    return "%s:%d:%s" % (_hexu(b.hash), b.psh_total, _fp(b.psh_hash))


def vote_validate_basic(v: Vote) -> Optional[str]:
    """Vote.ValidateBasic (types/vote.go:281-345)."""
    if v.type not in (H.PREVOTE_TYPE, H.PRECOMMIT_TYPE):
        return "invalid Type"
    if v.height < 0:
        return "negative Height"
    if v.round < 0:
        return "negative Round"
    b = v.block_id
    if b.hash and len(b.hash) != 32:
        return "wrong BlockID: wrong Hash: expected size to be 32 bytes, got %d bytes" % len(b.hash)
    if b.psh_hash and len(b.psh_hash) != 32:
        return ("wrong BlockID: wrong PartSetHeader: wrong Hash: expected size to be 32 bytes, got %d bytes" %
                len(b.psh_hash))
    nil = _block_id_is_nil(b)
    if not nil and not (len(b.hash) == 32 and b.psh_total > 0 and len(b.psh_hash) == 32):
        return "blockID must be either empty or complete, got: %s" % _block_id_string(b)
    if len(v.validator_address) != 20:
        return "expected ValidatorAddress size to be 20 bytes, got %d bytes" % len(v.validator_address)
    if v.validator_index < 0:
        return "negative ValidatorIndex"
    if not v.signature:
        return "signature is missing"
    if len(v.signature) > MAX_SIGNATURE_SIZE:
        return "signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
    if v.type != H.PRECOMMIT_TYPE or nil:
        if v.extension:
            return "unexpected vote extension"
        if v.extension_signature:
            return "unexpected vote extension signature"
    else:
        if len(v.extension_signature) > MAX_SIGNATURE_SIZE:
            return "vote extension signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
        if not v.extension_signature and v.extension:
            return "vote extension signature absent on vote with extension"
    return None


def _commit_sig_validate_basic(s) -> Optional[str]:
    """CommitSig.ValidateBasic (types/block.go:657-694)."""
    if s.block_id_flag not in (H.BLOCK_ID_FLAG_ABSENT, H.BLOCK_ID_FLAG_COMMIT, H.BLOCK_ID_FLAG_NIL):
        return "unknown BlockIDFlag: %d" % s.block_id_flag
    if s.block_id_flag == H.BLOCK_ID_FLAG_ABSENT:
        if s.validator_address:
            return "validator address is present"
        if tuple(s.timestamp) != H.ZERO_TIME:
            return "time is present"
        if s.signature:
            return "signature is present"
        return None
    if len(s.validator_address) != 20:
        return "expected ValidatorAddress size to be 20 bytes, got %d bytes" % len(s.validator_address)
    if not s.signature:
        return "signature is missing"
    if len(s.signature) > MAX_SIGNATURE_SIZE:
        return "signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
    return None


def extended_commit_sig_validate_basic(s: H.ExtendedCommitSig) -> Optional[str]:
    """ExtendedCommitSig.ValidateBasic (types/block.go:751-770)."""
    err = _commit_sig_validate_basic(s)
    if err:
        return err
    if s.block_id_flag == H.BLOCK_ID_FLAG_COMMIT:
        if len(s.extension) > MAX_VOTE_EXTENSION_SIZE:
            return "vote extension is too big (max: %d)" % MAX_VOTE_EXTENSION_SIZE
        if len(s.extension_signature) > MAX_SIGNATURE_SIZE:
            return "vote extension signature is too big (max: %d)" % MAX_SIGNATURE_SIZE
        return None
    if not s.extension_signature and s.extension:
        return "vote extension signature absent on vote with extension"
    return None


def extended_commit_sig_ensure_extension(s: H.ExtendedCommitSig) -> Optional[str]:
    """ExtendedCommitSig.EnsureExtension (types/block.go:774-779)."""
    if s.block_id_flag == H.BLOCK_ID_FLAG_COMMIT and not s.extension_signature:
        return "vote extension data is missing"
    return None


def extended_commit_validate_basic(ec: H.ExtendedCommit) -> Optional[str]:
    """ExtendedCommit.ValidateBasic (types/block.go:1206-1229)."""
    if ec.height < 0:
        return "negative Height"
    if ec.round < 0:
        return "negative Round"
    if ec.height >= 1:
        if _block_id_is_nil(ec.block_id):
            return "commit cannot be for nil block"
        if not ec.extended_signatures:
            return "no signatures in commit"
        for i, s in enumerate(ec.extended_signatures):
            err = extended_commit_sig_validate_basic(s)
            if err:
                return "wrong ExtendedCommitSig #%d: %s" % (i, err)
    return None


def extended_commit_ensure_extensions(ec: H.ExtendedCommit) -> Optional[str]:
    """ExtendedCommit.EnsureExtensions (types/block.go:1096-1103)."""
    for s in ec.extended_signatures:
        err = extended_commit_sig_ensure_extension(s)
        if err:
            return err
    return None


def get_extended_vote(ec: H.ExtendedCommit, idx: int) -> Vote:
    """ExtendedCommit.GetExtendedVote (types/block.go:1138-1152)."""
    s = ec.extended_signatures[idx]
    bid = ec.block_id if s.block_id_flag == H.BLOCK_ID_FLAG_COMMIT else H.BlockID()
    return Vote(H.PRECOMMIT_TYPE, ec.height, ec.round, bid, tuple(s.timestamp), s.validator_address, idx, s.signature,
                s.extension, s.extension_signature)


def extended_commits_to_vote_sets(jobs, verify_extended: VerifyFn):
    """ExtendedCommit.ToExtendedVoteSet (types/block.go:1037-1071) as
    votesFromExtendedCommit runs it (internal/consensus/state.go:722-732), for
    many jobs = (chain_id, validator set, extended commit) at once: what a
    node does with its stored extended commit when it starts or leaves
    blocksync.  The vote and extension signatures of ALL jobs are verified in
    one `verify_extended` call (one per chain_id, if the jobs name several);
    each job is then walked in the reference's order and yields its VoteSet,
    or the text of the panic / error the reference would have ended with."""
    plans = []
    by_chain: Dict[str, list] = {}
    for j, (chain_id, vals, ec) in enumerate(jobs):
        if ec.height == 0:  # NewVoteSet (types/vote_set.go:77-79)
            plans.append((None, [], "Cannot make VoteSet for height == 0, doesn't make sense."))
            continue
        vs = VoteSet(chain_id, ec.height, ec.round, H.PRECOMMIT_TYPE, vals, None, True, verify_extended)
        steps = []  # (vote, validate-basic error, pre-signature result, index among the chain's candidates)
        for idx, s in enumerate(ec.extended_signatures):
            if s.block_id_flag == H.BLOCK_ID_FLAG_ABSENT:
                continue
            v = get_extended_vote(ec, idx)
            bad = vote_validate_basic(v)
            if bad is not None:
                steps.append((v, bad, None, -1))
                break  # the reference panics here
            pre = vs._precheck(v)
            at = -1
            if pre is None:
                val = vals.validators[v.validator_index]
                c = by_chain.setdefault(chain_id, [[], []])
                at = len(c[0])
                c[0].append(v)
                c[1].append((val.key_kind, val.pub_key))
            steps.append((v, None, pre, at))
        plans.append((vs, steps, None))
    results = {c: verify_extended(c, vk[0], vk[1]) for c, vk in by_chain.items()}
    out = []
    for (chain_id, _, _), (vs, steps, text) in zip(jobs, plans):
        if text is None:
            for v, bad, pre, at in steps:
                if bad is not None:
                    text = "failed to validate vote reconstructed from LastCommit: " + bad
                    break
                added, err = pre if pre is not None else vs._add_checked(v, results[chain_id][at])
                if not added or err is not None:
                    text = "failed to reconstruct vote set from extended commit: " + (
                        err if err is not None else "%!w(<nil>)")
                    break
            if text is None and not vs.has_two_thirds_majority():
                text = "extended commit does not have +2/3 majority"
        out.append(text if text is not None else vs)
    return out
