"""Callers of the verification engine, driven with cross-commit batching
 — the reference loops that feed the
signature path one header / block at a time:

  * light.Client.verifySequential (light/client.go:554-634): VerifyAdjacent
    per height (light/verifier.go:106-155)
  * light.Client.verifySkipping (light/client.go:647-727): light.Verify
    (light/verifier.go:158-177) against a bisection cache of pivots
  * blocksync Reactor.poolRoutine (internal/blocksync/reactor.go:549-645):
    state.Validators.VerifyCommitLight(firstID, second.LastCommit), then
    ValidateBlock(first) -> state.LastValidators.VerifyCommit(
    state.LastBlockID, first.Height-1, first.LastCommit)
    (internal/state/validation.go:86-96)

The light checks run entirely in the engine's C++ host layer
(tmv_light_verify_many: Header.Hash and ValidatorSet.Hash of a whole window
on the device, SignedHeader.ValidateBasic, the trusting period / clock drift
checks and every commit check of the window in one signature batch); the
drivers here only decide which checks form a window and walk the results in
the reference's order, so the first error returned is the one the
one-at-a-time loop returns.  Primary/witness handling (provider I/O,
detector) is out of scope (networking).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

from . import host as H
from .host import LightBlock, LightJob, SignedHeader  # noqa: F401  (re-exported)

# light/client.go:45-46
SKIPPING_NUM, SKIPPING_DEN = 9, 16


@dataclass
class VerificationFailed:
    """light.ErrVerificationFailed (light/errors.go:53-66): the class and text
    of the wrapped error (TMV_LIGHT_*), the heights it failed between."""
    from_height: int
    to_height: int
    kind: int
    reason: str

    def __str__(self) -> str:
        return "verify from #%d to #%d failed: %s" % (self.from_height, self.to_height, self.reason)


def validator_set_arrays(sets: List[H.ValidatorSet]):
    """Column arrays of tmv_validator_set_hashes for `sets` (set order kept)."""
    import numpy as np
    vals = [v for vs in sets for v in vs.validators]
    n = len(vals)
    pk = np.frombuffer(b"".join(v.pub_key for v in vals), np.uint8) if n else np.zeros(0, np.uint8)
    kind = np.fromiter((v.key_kind for v in vals), np.uint8, count=n)
    power = np.fromiter((v.voting_power for v in vals), np.int64, count=n)
    off = np.zeros(len(sets) + 1, np.uint32)
    off[1:] = np.cumsum([len(vs.validators) for vs in sets])
    return pk, kind, power, off


def validator_set_hashes(ctx, sets: List[H.ValidatorSet]) -> List[bytes]:
    """ValidatorSet.Hash (types/validator_set.go:344-350) of each set, one GPU call."""
    if not sets:
        return []
    out = ctx.validator_set_hashes(*validator_set_arrays(sets))
    return [bytes(r) for r in out]


def in_order(windows, run, depth: int):
    """run(w) for each window with up to `depth` windows in flight on caller
    threads, results yielded in window order.  The engine calls release the
    GIL, so one window's conversion and engine call overlap another's.
    Windows are independent (each is built from inputs only, never from an
    earlier window's result), so a later window verified before an earlier
    one fails only costs work: the consumer stops at the first error and
    what ran past it is discarded -- the results equal one window at a
    time.  A consumer that stops early cancels the windows not yet started
    and waits for the running ones."""
    if depth <= 1:
        for w in windows:
            yield run(w)
        return
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    q = deque()
    with ThreadPoolExecutor(depth) as ex:
        try:
            for w in windows:
                q.append(ex.submit(run, w))
                if len(q) >= depth:
                    yield q.popleft().result()
            while q:
                yield q.popleft().result()
        finally:
            for f in q:
                f.cancel()


def verify_sequential(ctx, trusted: LightBlock, blocks: List[LightBlock], trusting_period_ns: int,
                      now: Tuple[int, int], max_clock_drift_ns: int = 10 * 10**9, window: int = 1000,
                      verify_many=None, depth: Optional[int] = None) -> Tuple[int, Optional[VerificationFailed]]:
    """Client.verifySequential over `blocks` (heights trusted+1, ...) with a
    single primary: VerifyAdjacent(verified, interim) per height, `window`
    headers per engine call (the light client's prefetch), `depth` windows in
    flight (default 2 on the engine, 1 with a caller's `verify_many`; see
    in_order).  Returns (headers verified, first ErrVerificationFailed or
    None)."""
    if depth is None:
        depth = 1 if verify_many else 2
    if verify_many:
        run, prepare = verify_many, (lambda jobs: jobs)
    else:
        # the C structs are built on this thread (Python, under the GIL),
        # the engine calls on the in_order threads (GIL released)
        fn = H._setup_light(H._setup(H._native.lib())).tmv_light_verify_many
        run = lambda pj: H.run_light_jobs(fn, ctx.handle, pj)
        prepare = H.PreparedLightJobs

    def windows():
        for lo in range(0, len(blocks), window):
            p = trusted if lo == 0 else blocks[lo - 1]
            jobs = []
            for lb in blocks[lo:lo + window]:
                jobs.append(LightJob(p.signed_header, None, lb.signed_header, lb.vals, trusting_period_ns, now,
                                     max_clock_drift_ns, mode=H.LIGHT_ADJACENT))
                p = lb
            yield prepare(jobs)

    done = 0
    prev = trusted
    for lo, res in zip(range(0, len(blocks), window), in_order(windows(), run, depth)):
        chunk = blocks[lo:lo + window]
        for lb, (kind, text) in zip(chunk, res):
            if kind != H.LIGHT_OK:
                return done, VerificationFailed(prev.height, lb.height, kind, text)
            prev = lb
            done += 1
    return done, None


def verify_sequential_wire(ctx, trusted: LightBlock, raws: List[bytes], trusting_period_ns: int,
                           now: Tuple[int, int], max_clock_drift_ns: int = 10 * 10**9, window: int = 1000,
                           verify_many=None, depth: Optional[int] = None, lib=None
                           ) -> Tuple[int, Optional[VerificationFailed]]:
    """verify_sequential over light blocks as the light store and peers hold
    them: `raws` holds each light block's protobuf bytes (tmproto.LightBlock,
    heights trusted+1, ...), nothing is decoded by the caller.  Per window one
    tmv_light_blocks_validate_wire call (H.light_blocks_validate_wire) yields
    the views, and the light jobs take signed header and validator set by
    pointer (H.ViewSignedHeader, H.ViewValidatorSet).  verify_many / depth as
    for verify_sequential; lib: the library of the wire call.  Returns what
    verify_sequential returns on the decoded blocks.  A light block whose
    bytes the strict scanner hands back, or that has no
    header, ends the run at its place with a LIGHT_ERR_OTHER "light block wire
    not handled: <reason name>": the reference would decode it and go on, and
    this model has no Go decoder to fall back to."""
    if depth is None:
        depth = 1 if verify_many else 2
    if verify_many:
        light, prepare = verify_many, (lambda jobs: jobs)
    else:
        fn = H._setup_light(H._setup(H._native.lib())).tmv_light_verify_many
        light = lambda pj: H.run_light_jobs(fn, ctx.handle, pj)
        prepare = H.PreparedLightJobs
    chain_id = trusted.signed_header.header.chain_id

    def run(w):
        pj, stop = w
        return light(pj), stop

    # a window's views come from its own bytes, but its first job's trusted
    # header is the window before's last block: the windows are built in order
    # on this thread, the engine calls run on the in_order threads
    def windows():
        p = trusted
        for lo in range(0, len(raws), window):
            vs = H.light_blocks_validate_wire(ctx, chain_id, raws[lo:lo + window], lib, decode=True)
            jobs, stop = [], None
            for v in vs:
                sh = v.signed_header
                if v.result == H.WIRE_NOT_HANDLED or sh is None or not sh.ptr.contents.header:
                    stop = "light block wire not handled: " + (v.reason if v.result == H.WIRE_NOT_HANDLED
                                                               else "MISSING")
                    break
                lb = LightBlock(sh, v.vals)
                jobs.append(LightJob(p.signed_header, None, sh, v.vals, trusting_period_ns, now, max_clock_drift_ns,
                                     mode=H.LIGHT_ADJACENT))
                p = lb
            yield prepare(jobs), (jobs, stop)
            if stop is not None:
                return

    done = 0
    prev_height = trusted.height
    for res, (jobs, stop) in in_order(windows(), run, depth):
        for jb, (kind, text) in zip(jobs, res):
            if kind != H.LIGHT_OK:
                return done, VerificationFailed(prev_height, jb.untrusted.height, kind, text)
            prev_height = jb.untrusted.height
            done += 1
        if stop is not None:
            return done, VerificationFailed(prev_height, prev_height + 1, H.LIGHT_ERR_OTHER, stop)
    return done, None


def _hex_upper(b: Optional[bytes]) -> str:
    return (b or b"").hex().upper()


def statesync_backfill(ctx, chain_id: str, raws: List[bytes], trusted_block_id_hash: bytes, window: int = 600,
                       start_height: Optional[int] = None, lib=None
                       ) -> Tuple[int, Optional[Tuple[int, str]], List[int]]:
    """Statesync's backfill (internal/statesync/reactor.go:437-600) over light
    blocks as peers deliver them, newest height first: `raws` holds the
    tmproto.LightBlock bytes of heights start_height, start_height - 1, ...
    (start_height: default the first block's own height), and
    trusted_block_id_hash is the trusted BlockID's hash for the first of them.
    One tmv_light_blocks_validate_wire call per window; then per block, in the
    reference's order: LightBlock.ValidateBasic(chain_id) and the height
    (reactor.go:511-523, "received invalid light block: ..."), Header.Hash
    against the running trusted hash (reactor.go:550-560, "received invalid
    light block. Expected hash %v, got: %v"), then trusted =
    header.LastBlockID.Hash.  There is no signature check in this loop.
    Returns (light blocks accepted, None or (height, text) of the first
    failure, the heights at which ValidatorsHash != NextValidatorsHash,
    reactor.go:569-577: counted from the second accepted block on, as the
    reference's lastValidatorSet is nil for the first).  The reference retries
    a failed height with another peer; this model stops there.  A light block
    that the strict scanner hands back ends it with
    "light block wire not handled: <reason name>"."""
    trusted = trusted_block_id_hash
    done, changes = 0, []
    height = start_height
    for lo in range(0, len(raws), window):
        for v in H.light_blocks_validate_wire(ctx, chain_id, raws[lo:lo + window], lib, decode=True):
            if v.result == H.WIRE_NOT_HANDLED:
                return done, (height if height is not None else 0, "light block wire not handled: " + v.reason), changes
            got = v.signed_header.height if v.result == H.WIRE_OK else None
            if height is None and got is not None:
                height = got
            if v.result != H.WIRE_OK or got != height:
                err = v.error if v.result != H.WIRE_OK else "%!w(<nil>)"  # fmt.Errorf("...%w", nil)
                return done, (height if height is not None else 0, "received invalid light block: " + err), changes
            if trusted != v.hash:
                return done, (height, "received invalid light block. Expected hash %s, got: %s"
                              % (_hex_upper(trusted), _hex_upper(v.hash))), changes
            hdr = v.signed_header.header
            if done > 0 and hdr.validators_hash != hdr.next_validators_hash:
                changes.append(height)
            trusted = hdr.last_block_id.hash
            done += 1
            height -= 1
    return done, None, changes


def schedule(last_verified: int, last_failed: int) -> int:
    """Client.schedule (light/client.go:721-725)."""
    return last_verified + (last_failed - last_verified) * SKIPPING_NUM // SKIPPING_DEN


def verify_skipping(ctx, trusted: LightBlock, target: LightBlock, provider: Callable[[int], LightBlock],
                    trusting_period_ns: int, now: Tuple[int, int], max_clock_drift_ns: int = 10 * 10**9,
                    trust: Tuple[int, int] = (1, 3), speculate: int = 8, verify_many=None
                    ) -> Tuple[Optional[List[int]], Optional[VerificationFailed]]:
    """Client.verifySkipping (light/client.go:647-727): bisection from the
    trusted block towards `target`, pivots from `provider(height)`.  The
    reference verifies one candidate per step; here every step verifies the
    current candidate, the rest of the cache and up to `speculate` further
    pivots (the heights schedule() would request next) in ONE engine call, and
    the results are consumed in the reference's order, so the trace and the
    error equal the reference's.  A provider error on a speculative pivot
    only stops the speculation; on a pivot the reference requests it is
    returned as ErrVerificationFailed{verified, pivot, err}
    (light/client.go:706-709).  Returns (trace heights, None) or
    (None, ErrVerificationFailed)."""
    run = verify_many or (lambda jobs: H.light_verify_many(ctx, jobs))
    cache = [target]
    fetched: Dict[int, LightBlock] = {}
    refused: Dict[int, Exception] = {}  # speculative fetches that failed (asked again only when needed)
    depth = 0
    verified = trusted
    trace = [trusted.height]
    results: Dict[Tuple[int, int], Tuple[int, Optional[str]]] = {}

    def block_at(h: int) -> LightBlock:
        if h not in fetched:
            fetched[h] = provider(h)
        return fetched[h]

    def speculative(h: int) -> Optional[LightBlock]:
        """A pivot the reference may never request: a provider error only
        ends the speculation (the reference would not have seen it)."""
        if h in refused:
            return None
        try:
            return block_at(h)
        except Exception as e:  # noqa: BLE001 -- any provider failure
            refused[h] = e
            return None

    while True:
        cand = cache[depth]
        key = (id(verified), id(cand))
        if key not in results:
            batch = list(cache[depth:])
            last = cache[-1].height
            for _ in range(speculate):
                p = schedule(verified.height, last)
                if p <= verified.height or p >= last:
                    break
                b = speculative(p)
                if b is None:
                    break
                batch.append(b)
                last = p
            # the client passes the verified block's own validator set
            # (light/client.go:680-681)
            jobs = [LightJob(verified.signed_header, verified.vals, b.signed_header, b.vals,
                             trusting_period_ns, now, max_clock_drift_ns, trust) for b in batch]
            for b, r in zip(batch, run(jobs)):
                results[(id(verified), id(b))] = r
        kind, text = results[key]
        if kind == H.LIGHT_OK:
            if depth == 0:
                trace.append(target.height)
                return trace, None
            verified = cand
            cache = cache[:depth]
            depth = 0
            trace.append(verified.height)
        elif kind == H.LIGHT_ERR_CANT_TRUST:
            if depth == len(cache) - 1:
                pivot = schedule(verified.height, cache[depth].height)
                refused.pop(pivot, None)  # the reference requests this one: ask again
                try:
                    cache.append(block_at(pivot))
                except Exception as e:  # noqa: BLE001 -- light/client.go:706-709
                    return None, VerificationFailed(verified.height, pivot, H.LIGHT_ERR_OTHER, str(e))
            depth += 1
        else:
            return None, VerificationFailed(verified.height, cand.height, kind, text)


@dataclass
class Block:
    """The parts of a types.Block blocksync's checks read."""
    height: int
    block_id: H.BlockID               # BlockID{Hash: block.Hash(), PartSetHeader}
    last_commit: Optional[H.Commit]   # the commit for height-1 carried by this block


def blocksync_replay(ctx, chain_id: str, vals: H.ValidatorSet, blocks: List[Block], last_block_id: H.BlockID,
                     initial_height: int = 1, window: int = 600, depth: Optional[int] = None,
                     verify_commits=None) -> Tuple[int, Optional[Tuple[int, str]]]:
    """poolRoutine's checks for each block pair (first, second) over a static
    validator set (state.Validators == state.LastValidators):
      light: vals.VerifyCommitLight(chainID, first.BlockID, first.Height, second.LastCommit)
      full:  ValidateBlock(first): at state.InitialHeight the LastCommit must
             carry no signatures, else vals.VerifyCommit(chainID,
             state.LastBlockID, first.Height-1, first.LastCommit)
    with state.LastBlockID = `last_block_id` for the first block and the
    previous block's BlockID after it (ApplyBlock).  `window` blocks per
    engine call (the pool buffers up to 600, internal/blocksync/pool.go:32-35);
    a commit read light at height H and full at H+1 is the same object, so its
    signatures are verified once; `depth` windows in flight (in_order;
    default 2 on the engine, 1 with a caller's `verify_commits`, a function
    jobs -> per-job error or None).  Returns (blocks applied, (height,
    error))."""
    if depth is None:
        depth = 1 if verify_commits else 2
    if verify_commits:
        prepare = lambda jobs: jobs

        def run(w):
            return w[:3], verify_commits(w[3])
    else:
        prepare = H.PreparedJobs

        def run(w):  # the C structs were built on the caller's thread (windows())
            H.run_prepared_jobs(ctx, w[3])
            return w[:3], w[3].decode()

    def windows():
        state_last = last_block_id
        for lo in range(0, len(blocks) - 1, window):
            chunk = blocks[lo:lo + window + 1]
            jobs, where, early = [], [], {}
            for i in range(len(chunk) - 1):
                first, second = chunk[i], chunk[i + 1]
                where.append((first.height, len(jobs)))
                jobs.append(H.CommitJob(H.MODE_LIGHT, chain_id, vals, first.block_id, first.height,
                                        second.last_commit))
                if first.height == initial_height:
                    if first.last_commit is not None and first.last_commit.signatures:
                        early[first.height] = "initial block can't have LastCommit signatures"
                    jobs.append(None)
                else:
                    jobs.append(H.CommitJob(H.MODE_FULL, chain_id, vals, state_last, first.height - 1,
                                            first.last_commit))
                state_last = first.block_id
            yield jobs, where, early, prepare([j for j in jobs if j is not None])

    applied = 0
    for (jobs, where, early), res in in_order(windows(), run, depth):
        it = iter(res)
        flat = [next(it) if j is not None else None for j in jobs]
        for height, k in where:
            err = flat[k] or early.get(height) or flat[k + 1]
            if err is not None:
                return applied, (height, err)
            applied += 1
    return applied, None


def _block_id_string(b: H.BlockID) -> str:
    """BlockID.String (types/block.go:1413-1415, part_set.go:100-102)."""
    return "%s:%d:%s" % (b.hash.hex().upper(), b.psh_total, (b.psh_hash + b"\0" * 6)[:6].hex().upper())


def blocksync_replay_full(ctx, chain_id: str, vals: H.ValidatorSet, blocks: List[H.FullBlock],
                          last_block_id: H.BlockID, initial_height: int = 1, window: int = 600,
                          depth: Optional[int] = None, part_size: int = 65536, verify_commits=None, lib=None,
                          vals_hash: Optional[bytes] = None, last_block_height: int = 0
                          ) -> Tuple[int, Optional[Tuple[int, str]]]:
    """poolRoutine's checks for each block pair (first, second)
    (internal/blocksync/reactor.go:563-586) over a static validator set, with
    nothing taken on trust from the caller: per window of `window` blocks
      * firstID = BlockID{first.Hash(), first.MakePartSet(part_size).Header()}:
        the hash from tmv_blocks_validate_basic (Header.Hash on the device),
        the part-set header from `raw` through tmv_part_set_headers (a block
        without `raw` is a ValueError);
      * vals.VerifyCommitLight(chainID, firstID, first.Height, second.LastCommit);
      * validateBlock(first) (internal/state/validation.go:14-96), in its order:
        Block.ValidateBasic (the three header hashes recomputed on the device),
        wrong Block.Header.ChainID, wrong Block.Header.Height, wrong
        Block.Header.LastBlockID, wrong Block.Header.ValidatorsHash, wrong
        Block.Header.NextValidatorsHash (both against the static set's hash,
        computed once, or `vals_hash`), then at the initial height "initial
        block can't have LastCommit signatures", else vals.VerifyCommit(chainID,
        state.LastBlockID, first.Height-1, first.LastCommit).
    state.LastBlockID is `last_block_id` and state.LastBlockHeight
    `last_block_height` before the first block, and the previous block's
    afterwards (ApplyBlock).  Not checked here, because they need
    application state: Block.Header.Version, AppHash, ConsensusHash and
    LastResultsHash, the proposer check (Validators.HasAddress), the block
    time checks and the evidence size limit -- blocksync_replay_stateful runs
    them too -- and the evidence's own ValidateBasic.
    `depth` windows in flight (in_order; default 2 on the engine, 1 with a
    caller's `verify_commits`, a function jobs -> per-job error or None);
    `lib`: the host layer to call (the CPU tests pass a build without the
    engine, with ctx = None).  Returns (blocks applied, (height, error) or
    None); the first error is the one the one-at-a-time loop returns."""
    return _replay_validated(ctx, chain_id, vals, blocks, last_block_id, initial_height, window, depth, part_size,
                             verify_commits, lib, vals_hash, last_block_height, "blocksync_replay_full")


def blocksync_replay_wire(ctx, chain_id: str, vals: H.ValidatorSet, raws: List[bytes], last_block_id: H.BlockID,
                          initial_height: int = 1, window: int = 600, depth: Optional[int] = None,
                          part_size: int = 65536, verify_commits=None, lib=None, vals_hash: Optional[bytes] = None,
                          last_block_height: int = 0) -> Tuple[int, Optional[Tuple[int, str]]]:
    """blocksync_replay_full over the blocks as a peer delivers them: `raws`
    holds each block's protobuf bytes (bcproto.BlockResponse.block), nothing is
    decoded by the caller.  The same loop, with Block.ValidateBasic, the block
    hashes, the part-set headers and the headers and commits that the other
    checks read all taken from one tmv_blocks_validate_wire call per window
    (H.blocks_validate_wire: one upload of the window's bytes).  Returns what
    blocksync_replay_full returns on the decoded blocks.  A block whose bytes
    the strict scanner hands back ends the replay at its
    height with "block wire not handled: <reason name>": the reference would
    decode it and go on, and this model has no Go decoder to fall back to."""
    return _replay_validated(ctx, chain_id, vals, raws, last_block_id, initial_height, window, depth, part_size,
                             verify_commits, lib, vals_hash, last_block_height, "blocksync_replay_wire", wire=True)


def _wire_window(ctx, lib, raws, part_size, height_before):
    """One window of blocksync_replay_wire: (decoded blocks, basic, psh) as
    _replay_validated reads them, a block that was not handled as (height it
    should have, text) in place of the decoded block."""
    vs = H.blocks_validate_wire(ctx, raws, part_size, lib, decode=True)
    blocks, height = [], height_before
    for v in vs:
        height = v.block.height if v.block is not None else (height or 0) + 1
        blocks.append(v.block if v.block is not None else (height, "block wire not handled: " + v.reason))
    return blocks, [(v.error, v.hash) for v in vs], [v.part_set_header for v in vs]


def _replay_validated(ctx, chain_id, vals, blocks, last_block_id, initial_height, window, depth, part_size,
                      verify_commits, lib, vals_hash, last_block_height, who, stateful=None, wire=False):
    """The replay loop of blocksync_replay_full; with `stateful` (a
    _StatefulChecks) also validateBlock's state-dependent checks, each at its
    place in the reference's order; with `wire`, `blocks` holds the blocks'
    protobuf bytes (blocksync_replay_wire).  A stateful that is a
    _DynamicChecks supplies the validator sets and their hashes block by block
    (blocksync_replay_dynamic); `vals` and `vals_hash` are then unused."""
    dynamic = stateful if isinstance(stateful, _DynamicChecks) else None
    n_apply = len(blocks) - 1 if dynamic is None else min(len(blocks) - 1, dynamic.limit)
    for b in blocks[:-1]:
        if not wire and b.raw is None:
            raise ValueError("%s: block %d has no raw bytes" % (who, b.height))
    if depth is None:
        depth = 1 if verify_commits else 2
    if vals_hash is None and dynamic is None:
        vals_hash = validator_set_hashes(ctx, [vals])[0]
    check = verify_commits or (lambda jobs: H.verify_commits(ctx, jobs))

    def run(lo):
        # the previous block rides along: its BlockID is state.LastBlockID of the window's first block
        first_of = max(lo - 1, 0)
        end = min(lo + window, n_apply)
        if wire:  # the window's last pair needs its second block decoded as well
            decoded, basic, psh = _wire_window(ctx, lib, blocks[first_of:end + 1], part_size,
                                               last_block_height if first_of == 0 else None)
            firsts = decoded[:-1]
        else:
            firsts, decoded = blocks[first_of:end], blocks[first_of:end + 1]
            basic = H.blocks_validate_basic(ctx, firsts, lib)
            psh = H.part_set_headers(ctx, [b.raw for b in firsts], part_size, lib)
        before = stateful.window(ctx, lib, first_of, len(firsts)) if stateful else None
        ids = [H.BlockID(hash_ or b"", total, phash) for (_, hash_), (total, phash) in zip(basic, psh)]
        out, jobs, slots = [], [], []
        for i in range(lo - first_of, len(firsts)):
            first, second = firsts[i], decoded[i + 1]
            g = first_of + i
            unhandled = first if isinstance(first, tuple) else second if isinstance(second, tuple) else None
            if unhandled is not None:  # wire only: ends the replay
                out.append(unhandled[0])
                slots.append((None, unhandled[1], None, None))
                break
            state_last = ids[i - 1] if g > 0 else last_block_id
            prev = firsts[i - 1] if g > 0 else None  # a tuple: not handled, and an earlier window has said so
            state_height = last_block_height if prev is None else prev[0] if isinstance(prev, tuple) else prev.height
            hd = first.header
            err = basic[i][0]
            # state.LastValidators, state.Validators and the two hashes a header must carry
            last_vals, cur_vals, cur_hash, next_hash = (dynamic.sets(g, before) if dynamic else
                                                        (vals, vals, vals_hash, vals_hash))
            if err is None and stateful:
                err = stateful.version(hd, g)
            if err is None and hd.chain_id != chain_id:
                err = "wrong Block.Header.ChainID. Expected %s, got %s" % (chain_id, hd.chain_id)
            if err is None and state_height == 0 and hd.height != initial_height:
                err = "wrong Block.Header.Height. Expected %d for initial block, got %d" % (hd.height, initial_height)
            if err is None and state_height > 0 and hd.height != state_height + 1:
                err = "wrong Block.Header.Height. Expected %d, got %d" % (state_height + 1, hd.height)
            if err is None and not hd.last_block_id.equals(state_last):
                err = "wrong Block.Header.LastBlockID.  Expected %s, got %s" % (_block_id_string(state_last),
                                                                              _block_id_string(hd.last_block_id))
            if err is None and stateful:
                err = stateful.app_info(hd, g, before)
            if err is None and hd.validators_hash != cur_hash:
                err = "wrong Block.Header.ValidatorsHash.  Expected %s, got %s" % (cur_hash.hex().upper(),
                                                                                 hd.validators_hash.hex().upper())
            if err is None and hd.next_validators_hash != next_hash:
                err = "wrong Block.Header.NextValidatorsHash.  Expected %s, got %s" % (
                    next_hash.hex().upper(), hd.next_validators_hash.hex().upper())
            light = len(jobs)
            jobs.append(H.CommitJob(H.MODE_LIGHT, chain_id, cur_vals, ids[i], hd.height, second.last_commit))
            full = None
            if err is None:
                if hd.height == initial_height:
                    if first.last_commit.signatures:
                        err = "initial block can't have LastCommit signatures"
                else:
                    full = len(jobs)
                    jobs.append(H.CommitJob(H.MODE_FULL, chain_id, last_vals, state_last, hd.height - 1,
                                            first.last_commit))
            late = stateful.after_commit(first, g, prev) if stateful and err is None else None
            if dynamic and err is None and late is None:  # validateBlock passed: ApplyBlock's state transition
                late = dynamic.transition_error(g)
            out.append((hd.height, ids[i], hd.time))
            slots.append((light, err, full, late))
        res = check(jobs)
        return [(h, (res[light] if light is not None else None) or err or
                 (res[full] if full is not None else None) or late)
                for h, (light, err, full, late) in zip(out, slots)]

    applied = 0
    for res in in_order(range(0, n_apply, window), run, depth):
        for at, err in res:
            height = at[0] if isinstance(at, tuple) else at
            if isinstance(err, Exception):  # the reference panics in this block's transition
                if dynamic:
                    dynamic.last_applied = None
                raise err
            if err is not None:
                return applied, (height, err)
            applied += 1
            if dynamic:
                dynamic.last_applied = at  # (height, BlockID, time) of the block: State.Update's arguments
    return applied, None


@dataclass
class ReplayState:
    """The parts of state.State (internal/state/state.go) that validateBlock
    reads, before the first block of a replay.  blocksync_replay_stateful runs
    over a static validator set (Validators == NextValidators ==
    LastValidators) and static consensus params, of which (Block.MaxBytes,
    Block.MaxGas) are hashed and Evidence.MaxBytes bounds a block's evidence.
    blocksync_replay_dynamic also reads next_validators and last_validators
    (None: `validators`), Validator.PubKeyTypes and the two heights of the last
    change, and returns a state with all of them filled."""
    chain_id: str
    validators: H.ValidatorSet
    app_hash: bytes
    last_results_hash: bytes
    last_block_id: H.BlockID = None
    last_block_height: int = 0
    last_block_time: Tuple[int, int] = (0, 0)   # the genesis time before the initial block
    initial_height: int = 1
    version_block: int = H.BLOCK_PROTOCOL
    version_app: int = 0
    block_max_bytes: int = 22020096
    block_max_gas: int = -1
    evidence_max_bytes: int = 1048576
    next_validators: Optional[H.ValidatorSet] = None
    last_validators: Optional[H.ValidatorSet] = None
    pub_key_types: List[str] = field(default_factory=lambda: ["ed25519"])
    last_height_validators_changed: int = 1
    last_height_consensus_params_changed: int = 1


@dataclass
class ConsensusParamUpdates:
    """The parts of a tmproto.ConsensusParams update that the replay reads;
    None: that message is absent from the update (UpdateConsensusParams,
    types/params.go:413-469, copies a present message whole)."""
    block: Optional[Tuple[int, int]] = None   # Block: (MaxBytes, MaxGas)
    evidence_max_bytes: Optional[int] = None  # Evidence.MaxBytes
    pub_key_types: Optional[List[str]] = None  # Validator.PubKeyTypes
    version_app: Optional[int] = None         # Version.AppVersion


@dataclass
class BlockRecord:
    """What the application answered for one block, as SaveFinalizeBlockResponses
    stores it: the tx results and the app hash after the block; for
    blocksync_replay_dynamic also the validator updates (host.ValidatorUpdate
    or (key kind, key, power)) and the consensus-param updates."""
    results: List[H.TxResult]
    app_hash: bytes
    validator_updates: List = field(default_factory=list)
    consensus_param_updates: Optional[ConsensusParamUpdates] = None


def go_time_string(t: Tuple[int, int]) -> str:
    """time.Time.String() of a UTC time (seconds, nanos): 2006-01-02
    15:04:05.999999999 +0000 UTC, the fraction trimmed and absent at zero nanos."""
    import datetime
    d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=t[0])
    frac = ("." + ("%09d" % t[1]).rstrip("0")) if t[1] else ""
    return "%04d-%02d-%02d %02d:%02d:%02d%s +0000 UTC" % (d.year, d.month, d.day, d.hour, d.minute, d.second, frac)


def _uvarint_len(u: int) -> int:
    n = 1
    while u >= 0x80:
        u >>= 7
        n += 1
    return n


def evidence_byte_size(evidence: List[bytes]) -> int:
    """EvidenceList.ByteSize (types/evidence.go:593-602): the size of
    tmproto.EvidenceList over the encoded items, 0 for none."""
    return sum(1 + _uvarint_len(len(e)) + len(e) for e in evidence)


class _StatefulChecks:
    """validateBlock's checks against state.State (internal/state/validation.go:
    21-27, 52-71, 98-135) for _replay_validated.  The state before block g is
    the caller's for g = 0 and follows from block g - 1 and its record
    afterwards (State.Update with no validator or param changes), so every
    window is built from inputs alone."""

    def __init__(self, state: ReplayState, blocks, records, lib):
        if len(records) < len(blocks) - 1:
            raise ValueError("blocksync_replay_stateful: %d records for %d blocks to apply"
                             % (len(records), len(blocks) - 1))
        self.st, self.blocks, self.records = state, blocks, records
        self.consensus_hash = H.consensus_params_hash(state.block_max_bytes, state.block_max_gas, lib)
        self.addresses = {v.address for v in state.validators.validators}
        self.evidence_max_bytes = state.evidence_max_bytes

    def window(self, ctx, lib, first_of: int, n: int) -> Tuple[int, List[bytes]]:
        """(first_of, LastResultsHash after each of blocks[first_of : first_of + n - 1]), one call."""
        lists = [self.records[j].results for j in range(first_of, first_of + n - 1)]
        return (first_of, H.results_hashes(ctx, lists, None, lib) if lists else [])

    def version(self, hd, g: int = 0) -> Optional[str]:
        st = self.st
        if hd.version_app != st.version_app or hd.version_block != st.version_block:
            return "wrong Block.Header.Version. Expected {%d %d}, got {%d %d}" % (
                st.version_block, st.version_app, hd.version_block, hd.version_app)
        return None

    def app_info(self, hd, g: int, before, consensus_hash: Optional[bytes] = None) -> Optional[str]:
        """consensus_hash: HashConsensusParams of the params in force (default: the state's)."""
        first_of, roots = before
        if consensus_hash is None:
            consensus_hash = self.consensus_hash
        app_hash = self.records[g - 1].app_hash if g > 0 else self.st.app_hash
        results_hash = roots[g - 1 - first_of] if g > 0 else self.st.last_results_hash
        for name, want, got in (("AppHash", app_hash, hd.app_hash), ("ConsensusHash", consensus_hash, hd.consensus_hash),
                                ("LastResultsHash", results_hash, hd.last_results_hash)):
            if want != got:
                return "wrong Block.Header.%s.  Expected %s, got %s" % (name, want.hex().upper(), got.hex().upper())
        return None

    def after_commit(self, block, g: int, prev=None, addresses=None, evidence_max_bytes: Optional[int] = None
                     ) -> Optional[str]:
        """prev: the block before (decoded; None for the first block of the
        replay).  addresses, evidence_max_bytes: state.Validators' addresses
        and the bound in force (default: the state's).  Nothing is stored on
        self: windows run on several threads."""
        st, hd = self.st, block.header
        if addresses is None:
            addresses = self.addresses
        if evidence_max_bytes is None:
            evidence_max_bytes = self.evidence_max_bytes
        if hd.proposer_address not in addresses:
            return "block.Header.ProposerAddress %s is not a validator" % hd.proposer_address.hex().upper()
        if g > 0 and not hasattr(prev, "header"):
            # the wire scanner handed the block before back: its own window has ended the replay there, and
            # this answer is never read; it is an error all the same, so that nothing passes unchecked
            return "block %d follows a block that was not handled" % hd.height
        last_time = st.last_block_time if g == 0 else prev.header.time
        if hd.height > st.initial_height:
            if not tuple(hd.time) > tuple(last_time):
                return "block time %s not greater than last block time %s" % (go_time_string(hd.time),
                                                                              go_time_string(last_time))
        elif hd.height == st.initial_height:
            if tuple(hd.time) < tuple(last_time):
                return "block time %s is before genesis time %s" % (go_time_string(hd.time), go_time_string(last_time))
        else:
            return "block height %d lower than initial height %d" % (hd.height, st.initial_height)
        got = evidence_byte_size(block.evidence)
        if got > evidence_max_bytes:
            return "Too much evidence: Max %d, got %d" % (evidence_max_bytes, got)
        return None


def blocksync_replay_stateful(ctx, state: ReplayState, blocks: List[H.FullBlock], records: List[BlockRecord],
                              window: int = 600, depth: Optional[int] = None, part_size: int = 65536,
                              verify_commits=None, lib=None, vals_hash: Optional[bytes] = None
                              ) -> Tuple[int, Optional[Tuple[int, str]]]:
    """blocksync_replay_full plus the rest of validateBlock
    (internal/state/validation.go:14-138): the checks that tie a header to the
    execution of the block before it, over a static validator set and static
    consensus params.  records[i] is what the application answered for
    blocks[i] (SaveFinalizeBlockResponses); after block h the state carries
    LastResultsHash = the merkle root over records[h].results with no leading
    leaf (internal/state/execution.go:262-267), AppHash = records[h].app_hash,
    LastBlockTime = h's time and LastBlockID (State.Update).  Per window all
    result roots come from one tmv_results_hash_many call beside the window's
    other launches; HashConsensusParams is computed once.  In the reference's
    order and with its texts, after VerifyCommitLight of the pair:
      <Block.ValidateBasic>
      wrong Block.Header.Version. Expected {B A}, got {B A}
      wrong Block.Header.ChainID / Height / LastBlockID        (as blocksync_replay_full)
      wrong Block.Header.AppHash.  Expected %X, got %X
      wrong Block.Header.ConsensusHash.  Expected %X, got %X
      wrong Block.Header.LastResultsHash.  Expected %X, got %X
      wrong Block.Header.ValidatorsHash / NextValidatorsHash   (as blocksync_replay_full)
      <LastCommit: the initial block's text or VerifyCommit>   (as blocksync_replay_full)
      block.Header.ProposerAddress %X is not a validator
      block time %v not greater than last block time %v        (height > initial)
      block time %v is before genesis time %v                  (height == initial)
      block height %v lower than initial height %v
      Too much evidence: Max %d, got %d
    Times print as Go's time.Time.String() in UTC.  Left to the caller:
    validator-set and consensus-param updates, the evidence's own verification,
    ValidateConsensusParams.  The other arguments and the return value are
    blocksync_replay_full's."""
    return _replay_validated(ctx, state.chain_id, state.validators, blocks, state.last_block_id or H.BlockID(),
                             state.initial_height, window, depth, part_size, verify_commits, lib, vals_hash,
                             state.last_block_height, "blocksync_replay_stateful",
                             _StatefulChecks(state, blocks, records, lib))


MAX_BLOCK_SIZE_BYTES = 104857600  # types/params.go:20
_KEY_SIZES = {H.TMV_KIND_ED25519: ("PubKeyEd25519", 32), H.TMV_KIND_SR25519: ("PubKeySr25519", 32),
              H.TMV_KIND_SECP256K1: ("PubKeySecp256k1", 33)}


def _update_string(u: H.ValidatorUpdate) -> str:
    return "{%s:%s %d}" % (H.KEY_TYPE_NAMES.get(u.key_kind, "kind%d" % u.key_kind), u.pub_key.hex().upper(), u.power)


def _key_error(u: H.ValidatorUpdate) -> Optional[str]:
    """encoding.PubKeyFromProto's errors (crypto/encoding/codec.go:49-78)."""
    if u.key_kind not in _KEY_SIZES:
        return "fromproto: key type %d is not supported" % u.key_kind
    name, size = _KEY_SIZES[u.key_kind]
    if len(u.pub_key) != size:
        return "invalid size for %s. Got %d, expected %d" % (name, len(u.pub_key), size)
    return None


def validate_validator_updates(updates: List[H.ValidatorUpdate], pub_key_types: List[str]) -> Optional[str]:
    """validateValidatorUpdates (internal/state/execution.go:501-524).  The
    reference prints the abci.ValidatorUpdate with %v, which renders a pointer;
    here it prints as {<key type>:<HEX key> <power>}."""
    for u in updates:
        if u.power < 0:
            return "voting power can't be negative %s" % _update_string(u)
        if u.power == 0:
            continue
        err = _key_error(u)
        if err is not None:
            return err
        if H.KEY_TYPE_NAMES[u.key_kind] not in pub_key_types:
            return "validator %s is using pubkey %s, which is unsupported for consensus" % (
                _update_string(u), H.KEY_TYPE_NAMES[u.key_kind])
    return None


@dataclass
class _Params:
    """The consensus params the replay reads."""
    block_max_bytes: int
    block_max_gas: int
    evidence_max_bytes: int
    version_app: int
    pub_key_types: List[str]

    def updated(self, u: ConsensusParamUpdates) -> "_Params":
        """UpdateConsensusParams over these fields."""
        p = _Params(self.block_max_bytes, self.block_max_gas, self.evidence_max_bytes, self.version_app,
                    self.pub_key_types)
        if u.block is not None:
            p.block_max_bytes, p.block_max_gas = u.block
        if u.evidence_max_bytes is not None:
            p.evidence_max_bytes = u.evidence_max_bytes
        if u.pub_key_types is not None:
            p.pub_key_types = list(u.pub_key_types)
        if u.version_app is not None:
            p.version_app = u.version_app
        return p

    def validate(self) -> Optional[str]:
        """ValidateConsensusParams (types/params.go:272-354) over these fields."""
        if self.block_max_bytes <= 0:
            return "block.MaxBytes must be greater than 0. Got %d" % self.block_max_bytes
        if self.block_max_bytes > MAX_BLOCK_SIZE_BYTES:
            return "block.MaxBytes is too big. %d > %d" % (self.block_max_bytes, MAX_BLOCK_SIZE_BYTES)
        if self.block_max_gas < -1:
            return "block.MaxGas must be greater or equal to -1. Got %d" % self.block_max_gas
        if self.evidence_max_bytes > self.block_max_bytes:
            return "evidence.MaxBytesEvidence is greater than upper bound, %d > %d" % (self.evidence_max_bytes,
                                                                                      self.block_max_bytes)
        if self.evidence_max_bytes < 0:
            return "evidence.MaxBytes must be non negative. Got: %d" % self.evidence_max_bytes
        if not self.pub_key_types:
            return "len(Validator.PubKeyTypes) must be greater than 0"
        for i, t in enumerate(self.pub_key_types):
            if t not in H.KEY_TYPE_NAMES.values():
                return "params.Validator.PubKeyTypes[%d], %s, is an unknown pubkey type" % (i, t)
        return None


class _Schedule:
    """The validator sets and consensus params of a replay, from the state and
    the records alone (no block is read): State.Update's part of the state,
    for every block up to the first one whose transition fails.

    With S[0], S[1], S[2] = the state's LastValidators, Validators,
    NextValidators and S[k + 3] = IncrementProposerPriority(1) of S[k + 2]
    updated with record k's changes, the state before block g holds
    LastValidators = S[g], Validators = S[g + 1], NextValidators = S[g + 2]:
    record k's updates first sign at block k + 2.  The members of a set change
    only where a record had updates (a `version`: one list of validators that
    every set of the version shares, so a window converts and hashes it once);
    between two changes only the priorities and the proposer move, and one
    validator_set_rotate call walks all of those blocks.  The whole schedule
    is built before the first window runs; a failure or a panic of record g is
    kept with g and comes up only when block g's own checks have passed."""

    def __init__(self, state: ReplayState, records, n_blocks: int, lib):
        self.lib = lib
        self.first = [state.last_validators or state.validators, state.validators,
                      state.next_validators or state.validators]
        self.version_of: List[int] = []       # per k: which list of members S[k] holds
        self.sets: List[H.ValidatorSet] = []  # per k: the version's validators with the proposer of S[k]
        self.members: List[H.ValidatorSet] = []  # per version: a set to hash
        self.base = {}                        # version -> (the set its rotation starts from, k of that set)
        key = lambda vs: [(v.pub_key, v.key_kind, v.voting_power) for v in vs.validators]  # noqa: E731
        for k, vs in enumerate(self.first):
            same = [j for j in range(k) if self.first[j] is vs or key(self.first[j]) == key(vs)]
            if same:  # the same members: one version to convert and hash, its own proposer
                self.version_of.append(self.version_of[same[0]])
            else:
                self.version_of.append(len(self.members))
                self.members.append(vs)
            self.sets.append(H.ValidatorSet(self.members[self.version_of[k]].validators, vs.proposer_index))
        self.base[self.version_of[2]] = (self.first[2], 2)
        self.params = [_Params(state.block_max_bytes, state.block_max_gas, state.evidence_max_bytes, state.version_app,
                               list(state.pub_key_types))]
        self.vals_changed = [state.last_height_validators_changed]  # LastHeightValidatorsChanged before block g
        self.params_changed = [state.last_height_consensus_params_changed]
        # (g, text): block g's transition fails; (g, ValidatorSetPanic): the reference panics in it
        self.failed: Optional[Tuple[int, object]] = None
        height = state.last_block_height + 1 if state.last_block_height else state.initial_height
        cur, version, pending, pending_from = self.first[2], self.version_of[2], 0, 0

        def flush():  # the rotations since the last change, in one call
            nonlocal cur, pending
            if pending:
                try:
                    cur, props = H.validator_set_rotate(cur, pending, 1, lib)
                except H.ValidatorSetPanic as e:  # a set that cannot rotate fails at its first rotation
                    self.failed = (pending_from, e)
                    return
                for p in props:
                    self.version_of.append(version)
                    self.sets.append(H.ValidatorSet(self.members[version].validators, p))
                pending = 0

        for g in range(n_blocks):
            rec = records[g]
            vals_changed, params_changed, p = self.vals_changed[g], self.params_changed[g], self.params[g]
            if rec.validator_updates:
                ups = [u if isinstance(u, H.ValidatorUpdate) else H.ValidatorUpdate(*u) for u in rec.validator_updates]
                err = validate_validator_updates(ups, p.pub_key_types)
                if err is not None:
                    self.failed = (g, "error in validator updates: " + err)
                    break
                err = next((e for e in map(_key_error, ups) if e is not None), None)  # PB2TM.ValidatorUpdates
                if err is not None:
                    self.failed = (g, err)
                    break
                flush()
                if self.failed is not None:
                    break
                try:
                    cur, err = H.validator_set_update(cur, ups, True, lib)
                except H.ValidatorSetPanic as e:
                    self.failed = (g, e)
                    break
                if err is not None:
                    self.failed = (g, "commit failed for application: changing validator set: " + err)
                    break
                version = len(self.members)
                self.members.append(cur)
                self.base[version] = (cur, g + 2)
                vals_changed = height + g + 2
            if rec.consensus_param_updates is not None:
                p = p.updated(rec.consensus_param_updates)
                err = p.validate()
                if err is not None:
                    self.failed = (g, "commit failed for application: updating consensus params: " + err)
                    break
                params_changed = height + g + 1
            if pending == 0:
                pending_from = g
            pending += 1  # S[g + 3]
            self.params.append(p)
            self.vals_changed.append(vals_changed)
            self.params_changed.append(params_changed)
        if self.failed is None or not isinstance(self.failed[1], H.ValidatorSetPanic):
            flush()  # the rotations before the block that failed, or the rest of the chain
        self.limit = self.failed[0] + 1 if self.failed else n_blocks  # the blocks whose checks run

    def set_at(self, k: int) -> H.ValidatorSet:
        """S[k] with its priorities and its proposer."""
        if k < 3:
            return H.ValidatorSet(list(self.first[k].validators), self.first[k].proposer_index)
        base, born = self.base[self.version_of[k]]
        return H.validator_set_rotate(base, k - born, 1, self.lib)[0]


class _DynamicChecks(_StatefulChecks):
    """_StatefulChecks against the state before each block, with the validator
    sets and the consensus params of a _Schedule."""

    def __init__(self, state: ReplayState, blocks, records, lib, set_hashes):
        if len(records) < len(blocks) - 1:
            raise ValueError("blocksync_replay_dynamic: %d records for %d blocks to apply"
                             % (len(records), len(blocks) - 1))
        self.st, self.blocks, self.records, self.lib = state, blocks, records, lib
        self.set_hashes = set_hashes
        self.schedule = sc = _Schedule(state, records, max(len(blocks) - 1, 0), lib)
        self.limit = sc.limit
        self.last_applied = None
        # read-only from here on (the windows run on several threads): HashConsensusParams of the params
        # before each block, and the addresses of each distinct set
        hashes: Dict[Tuple[int, int], bytes] = {}
        for p in sc.params:
            key = (p.block_max_bytes, p.block_max_gas)
            if key not in hashes:
                hashes[key] = H.consensus_params_hash(key[0], key[1], lib)
        self._consensus_hash = [hashes[(p.block_max_bytes, p.block_max_gas)] for p in sc.params]
        self._addresses = [frozenset(x.address for x in vs.validators) for vs in sc.members]

    def window(self, ctx, lib, first_of: int, n: int):
        """_StatefulChecks.window, and the hash of every distinct validator set
        that the window's blocks name, from one set_hashes call."""
        sc = self.schedule
        versions = sorted({sc.version_of[k] for k in range(first_of + 1, first_of + n + 2)})
        hashes = self.set_hashes([sc.members[v] for v in versions])
        return _StatefulChecks.window(self, ctx, lib, first_of, n) + (dict(zip(versions, hashes)),)

    def sets(self, g: int, before):
        sc, hashes = self.schedule, before[2]
        return sc.sets[g], sc.sets[g + 1], hashes[sc.version_of[g + 1]], hashes[sc.version_of[g + 2]]

    def version(self, hd, g: int = 0) -> Optional[str]:
        app = self.schedule.params[g].version_app
        if hd.version_app != app or hd.version_block != self.st.version_block:
            return "wrong Block.Header.Version. Expected {%d %d}, got {%d %d}" % (
                self.st.version_block, app, hd.version_block, hd.version_app)
        return None

    def app_info(self, hd, g: int, before) -> Optional[str]:
        return _StatefulChecks.app_info(self, hd, g, before[:2], self._consensus_hash[g])

    def after_commit(self, block, g: int, prev=None) -> Optional[str]:
        sc = self.schedule
        return _StatefulChecks.after_commit(self, block, g, prev, self._addresses[sc.version_of[g + 1]],
                                            sc.params[g].evidence_max_bytes)

    def transition_error(self, g: int) -> Optional[str]:
        f = self.schedule.failed
        return f[1] if f is not None and f[0] == g else None

    def state_after(self, applied: int, ctx) -> ReplayState:
        """The state after `applied` blocks (State.Update's result, with the
        AppHash that state.Save fills in)."""
        import dataclasses
        sc, st = self.schedule, self.st
        p = sc.params[applied]
        out = dataclasses.replace(
            st, last_validators=sc.set_at(applied), validators=sc.set_at(applied + 1),
            next_validators=sc.set_at(applied + 2), block_max_bytes=p.block_max_bytes, block_max_gas=p.block_max_gas,
            evidence_max_bytes=p.evidence_max_bytes, version_app=p.version_app, pub_key_types=list(p.pub_key_types),
            last_height_validators_changed=sc.vals_changed[applied],
            last_height_consensus_params_changed=sc.params_changed[applied],
            last_block_id=st.last_block_id or H.BlockID())
        if applied:
            height, block_id, time = self.last_applied
            rec = self.records[applied - 1]
            out = dataclasses.replace(out, last_block_height=height, last_block_id=block_id, last_block_time=tuple(time),
                                      app_hash=rec.app_hash,
                                      last_results_hash=H.results_hashes(ctx, [rec.results], None, self.lib)[0])
        return out


def mixed_set_hashes(ctx, sets: List[H.ValidatorSet], lib=None) -> List[bytes]:
    """ValidatorSet.Hash of each set: one validator_set_hashes call on the
    device over the sets of ed25519 and sr25519 keys; a set that holds a
    secp256k1 key (tmv_validator_set_hashes does not take those), and every
    set without a context, on the host (host.validator_set_hash_host)."""
    dev = [i for i, vs in enumerate(sets) if ctx is not None and all(
        v.key_kind in (H.TMV_KIND_ED25519, H.TMV_KIND_SR25519) and len(v.pub_key) == 32 for v in vs.validators)]
    out: List[Optional[bytes]] = [None] * len(sets)
    if dev:
        for i, h in zip(dev, validator_set_hashes(ctx, [sets[i] for i in dev])):
            out[i] = h
    return [h if h is not None else H.validator_set_hash_host(vs, lib) for h, vs in zip(out, sets)]


def blocksync_replay_dynamic(ctx, state: ReplayState, blocks, records: List[BlockRecord], window: int = 600,
                             depth: Optional[int] = None, part_size: int = 65536, verify_commits=None,
                             set_hashes=None, lib=None, wire: bool = False
                             ) -> Tuple[int, Optional[Tuple[int, str]], ReplayState]:
    """blocksync_replay_stateful across validator-set and consensus-param
    changes: the reference's ApplyBlock loop with State.Update
    (internal/state/execution.go:527-595) between the blocks.  blocks: the
    FullBlocks, or with wire=True their protobuf bytes (the window of
    blocksync_replay_wire).  records[i]: what the application answered for
    blocks[i], with its validator_updates and consensus_param_updates.

    Block g is checked against the state before it -- VerifyCommitLight of the
    pair by state.Validators, ValidatorsHash against state.Validators.Hash(),
    NextValidatorsHash against state.NextValidators.Hash(), LastCommit by
    state.LastValidators.VerifyCommit, the proposer by state.Validators, the
    version, ConsensusHash and the evidence bound by the params in force --
    with blocksync_replay_stateful's texts in its order.  Then the transition,
    whose failure ends the replay at g's height with g not applied:
      error in validator updates: voting power can't be negative {T:K P}
      error in validator updates: validator {T:K P} is using pubkey T, which is unsupported for consensus
      error in validator updates: invalid size for PubKeyEd25519. Got %d, expected %d   (and the other key types)
      commit failed for application: changing validator set: <UpdateWithChangeSet's text>
      commit failed for application: updating consensus params: <ValidateConsensusParams' text>
    The reference prints an abci.ValidatorUpdate with %v, which renders a
    pointer; here {T:K P} is {<key type>:<HEX key> <power>}.
    UpdateConsensusParams and ValidateConsensusParams cover the fields of
    ConsensusParamUpdates (block, evidence max bytes, pub key types, app
    version).  Updates of block h change NextValidators after h and first sign
    at h + 2; param updates hold from h + 1.  A change set on which the
    reference panics raises host.ValidatorSetPanic, once the replay has reached
    the block whose transition it belongs to (an earlier block that fails a
    check ends the replay with its own error first).

    The validator sets and params of every block follow from the state and the
    records alone (host.validator_set_update / validator_set_rotate, on the
    host), so the windows stay independent and `depth` of them are in flight.
    Per window: one `set_hashes` call (sets -> hashes; default
    mixed_set_hashes) over the window's distinct sets -- a set is new only
    where a record had updates -- and one commit batch (`verify_commits`).
    Not done here: evidence verification, vote extensions, the synchrony,
    timeout and ABCI params, LoadValidators' checkpoint rotation.

    Returns (blocks applied, (height, error) or None, the state after the
    applied blocks: the three validator sets with their priorities and
    proposers, the params, the heights of the last changes)."""
    if set_hashes is None:
        set_hashes = lambda sets: mixed_set_hashes(ctx, sets, lib)  # noqa: E731
    dyn = _DynamicChecks(state, blocks, records, lib, set_hashes)
    applied, err = _replay_validated(ctx, state.chain_id, None, blocks, state.last_block_id or H.BlockID(),
                                     state.initial_height, window, depth, part_size, verify_commits, lib, None,
                                     state.last_block_height, "blocksync_replay_dynamic", dyn, wire)
    return applied, err, dyn.state_after(applied, ctx)


# ---- merkle proofs: Txs.Hash / Txs.Proof (types/tx.go:30-75) ----

@dataclass
class MerkleProof:
    """merkle.Proof (crypto/merkle/proof.go:26-31)."""
    total: int
    index: int
    leaf_hash: bytes
    aunts: List[bytes]


def pack_items(items: List[bytes]):
    """(data, leaf_off) of tmv_merkle_roots / tmv_merkle_proofs for `items`."""
    import numpy as np
    off = np.zeros(len(items) + 1, np.uint32)
    off[1:] = np.cumsum([len(b) for b in items])
    return np.frombuffer(b"".join(items), np.uint8), off


def proofs_of_tree(total: int, leaf_hashes, aunt_off, aunts, first: int = 0) -> List[MerkleProof]:
    """The proofs of one tree out of Context.merkle_proofs' arrays: leaves
    [first, first + total)."""
    return [MerkleProof(total, i, bytes(leaf_hashes[first + i]),
                        [bytes(a) for a in aunts[int(aunt_off[first + i]):int(aunt_off[first + i + 1])]])
            for i in range(total)]


def txs_hash(ctx, txs: List[bytes]) -> bytes:
    """Txs.Hash (types/tx.go:34-39): the merkle root over SHA-256(tx), the
    transactions hashed on the device (TMV_MERKLE_PREHASH)."""
    from . import _native
    import numpy as np
    data, off = pack_items(txs)
    roots, _, _, _ = ctx.merkle_proofs(data, off, np.array([0, len(txs)], np.uint32),
                                       flags=_native.TMV_MERKLE_PREHASH, aunts=False)
    return bytes(roots[0])


def txs_proofs(ctx, txs: List[bytes]) -> Tuple[bytes, List[MerkleProof]]:
    """Txs.Proof (types/tx.go:61-70) for every transaction in one call: the
    root and the merkle.Proof of each SHA-256(tx)."""
    from . import _native
    import numpy as np
    data, off = pack_items(txs)
    roots, leaves, aoff, aunts = ctx.merkle_proofs(data, off, np.array([0, len(txs)], np.uint32),
                                                   flags=_native.TMV_MERKLE_PREHASH)
    return bytes(roots[0]), proofs_of_tree(len(txs), leaves, aoff, aunts)

