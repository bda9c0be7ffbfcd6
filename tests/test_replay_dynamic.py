"""chains.blocksync_replay_dynamic on the CPU: the host layer built without the
engine (tests/native/valset, libvalsethost.so) and the C++ commit verifier over
the C oracle's signature checks (tests/commit_fixtures.py), against the
one-block-at-a-time restatement of tests/valset_chain_cases.py.  The GPU twin
is tests/test_gpu_replay_dynamic.py."""
import ctypes
import dataclasses
import os

import pytest

import commit_fixtures as F
import valset_chain_cases as C
from tendermint_amd import chains, host as H
from tendermint_amd.testing.factory import _valset_hash

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libvalsethost.so")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def fake():
    fb = F.FakeBackend()
    fb.real_signatures(True)
    yield fb
    fb.real_signatures(False)


@pytest.fixture(scope="module")
def scenarios():
    return C.scenarios()


@pytest.fixture(scope="module")
def wanted(fake, scenarios):
    """The restatement's answer for every scenario, computed once."""
    return {name: C.replay_one_at_a_time(fake, st, bl, rec) for name, (st, bl, rec) in scenarios.items()}


def run(lib, fake, state, blocks, records, window, depth, wire=False, counts=None):
    def set_hashes(sets):
        if counts is not None:
            counts.append(len(sets))
        return [_valset_hash(vs) for vs in sets]
    return chains.blocksync_replay_dynamic(None, state, [b.raw for b in blocks] if wire else blocks, records,
                                           window=window, depth=depth, part_size=C.PART_SIZE, lib=lib, wire=wire,
                                           verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs),
                                           set_hashes=set_hashes)


def same(got, want):
    return got[:2] == want[:2] and C.same_state(C.state_dict(got[2]), want[2])


# what each scenario must end with: (blocks applied, height, a part of the text); None: the whole chain
EXPECTED = {
    "clean": (23, None, None),
    "stale_validators_hash": (5, 6, "wrong Block.Header.ValidatorsHash.  Expected "),
    "stale_next_validators_hash": (4, 5, "wrong Block.Header.NextValidatorsHash.  Expected "),
    "removed_proposer": (10, 11, "block.Header.ProposerAddress %s is not a validator" % C.signer("e1").address.hex().upper()),
    "signed_by_the_old_set": (5, 6, "Invalid commit -- wrong set size: 8 vs 7"),
    "other_key_signs": (14, 15, "pubkey is not Ed25519"),
    "tampered_signature": (6, 7, "wrong signature (#2): "),
    "negative_power": (2, 3, "error in validator updates: voting power can't be negative {ed25519:%s -3}"
                       % C.signer("e5").pub_key.hex().upper()),
    "unsupported_key_type": (2, 3, "error in validator updates: validator {secp256k1:%s 5} is using pubkey secp256k1, "
                             "which is unsupported for consensus" % C.signer("k0").pub_key.hex().upper()),
    "unknown_removal": (2, 3, "commit failed for application: changing validator set: failed to find validator %s to "
                        "remove" % C.signer("e9").address.hex().upper()),
    "emptying_the_set": (2, 3, "commit failed for application: changing validator set: applying the validator changes "
                         "would result in empty set"),
    "duplicate_update": (2, 3, "commit failed for application: changing validator set: duplicate entry Validator{"),
    "short_key": (2, 3, "error in validator updates: invalid size for PubKeyEd25519. Got 31, expected 32"),
    "block_max_bytes_zero": (2, 3, "commit failed for application: updating consensus params: block.MaxBytes must be "
                             "greater than 0. Got 0"),
    "evidence_above_block": (2, 3, "commit failed for application: updating consensus params: evidence.MaxBytesEvidence "
                             "is greater than upper bound, 22020097 > 22020096"),
    "max_gas_below": (2, 3, "commit failed for application: updating consensus params: block.MaxGas must be greater or "
                      "equal to -1. Got -2"),
    "no_key_types": (2, 3, "commit failed for application: updating consensus params: len(Validator.PubKeyTypes) must "
                     "be greater than 0"),
    "unknown_key_type": (2, 3, "commit failed for application: updating consensus params: "
                         "params.Validator.PubKeyTypes[1], bls, is an unknown pubkey type"),
    "set_before_params": (2, 3, "commit failed for application: changing validator set: failed to find validator "),
}


def test_the_restatement_gives_the_texts(scenarios, wanted):
    """Every scenario ends where it should, with the text of its cause, in the
    restatement: the driver tests below compare with that."""
    assert set(scenarios) == set(EXPECTED)
    for name, (applied, height, text) in EXPECTED.items():
        got = wanted[name]
        assert got[0] == applied, (name, got[:2])
        if height is None:
            assert got[1] is None, (name, got[1])
        else:
            assert got[1][0] == height and text in got[1][1], (name, got[1])


def test_the_chain_changes_as_planned(scenarios):
    """Seven validators at genesis; additions, removals, power changes, an
    sr25519 validator, two param updates."""
    state, blocks, records = scenarios["clean"]
    assert len(blocks) == C.N_BLOCKS and len(state.validators.validators) == C.N_VALS
    hashes = [b.header.validators_hash for b in blocks]
    changes_at = [g for g in range(1, len(blocks)) if hashes[g] != hashes[g - 1]]
    assert changes_at == [3, 5, 9, 12, 15, 22]  # record k's updates name Validators at block k + 2
    assert blocks[8].header.consensus_hash == blocks[9].header.consensus_hash != blocks[10].header.consensus_hash
    assert [b.header.version_app for b in blocks[14:18]] == [0, 0, 1, 1]
    assert any(u.key_kind == H.TMV_KIND_SR25519 for r in records for u in r.validator_updates)


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("window", [1, 2, 5, 600])
def test_replay_equals_one_at_a_time(lib, fake, scenarios, wanted, window, depth):
    for name, (state, blocks, records) in scenarios.items():
        got = run(lib, fake, state, blocks, records, window, depth)
        assert got[:2] == wanted[name][:2], name
        assert same(got, wanted[name]), name


@pytest.mark.parametrize("window", [1, 5, 600])
def test_replay_over_bytes(lib, fake, scenarios, wanted, window):
    for name in ("clean", "stale_validators_hash", "signed_by_the_old_set", "tampered_signature", "unknown_removal",
                 "removed_proposer"):
        state, blocks, records = scenarios[name]
        assert same(run(lib, fake, state, blocks, records, window, 2, wire=True), wanted[name]), name


@pytest.mark.parametrize("window", [1, 2, 5, 600])
def test_one_set_hash_call_per_window(lib, fake, scenarios, window):
    """One set_hashes call per window, over the window's distinct sets: the
    sets that a window's blocks name as LastValidators' successor chain
    (Validators, NextValidators), new only where a record had updates."""
    state, blocks, records = scenarios["clean"]
    counts = []
    assert run(lib, fake, state, blocks, records, window, 1, counts=counts)[:2] == (23, None)
    n = len(blocks) - 1
    starts = list(range(0, n, window))
    assert len(counts) == len(starts)
    # S[k] changes members at k = record + 3; S[0] is the empty genesis LastValidators, S[1] and S[2] one set
    born = [0, 1] + [k + 3 for k, (ups, _) in sorted(C.plan().items()) if ups]
    version = lambda k: max(i for i, b in enumerate(born) if b <= k)  # noqa: E731
    for lo, count in zip(starts, counts):
        first_of, end = max(lo - 1, 0), min(lo + window, n)
        assert count == len({version(k) for k in range(first_of + 1, end + 2)}), (lo, count)
    if window == 600:
        assert counts == [7]


def test_static_chain_equals_the_stateful_driver(lib, fake):
    """On records without updates the new driver returns what blocksync_replay_stateful returns."""
    import results_cases as RC
    for name, (state, blocks, records, _) in RC.replay_scenarios().items():
        vh = _valset_hash(state.validators)
        verify = lambda jobs: F.fake_verify_commits(fake, jobs)  # noqa: E731
        for window in (1, 5, 100):
            want = chains.blocksync_replay_stateful(None, state, blocks, records, window=window, part_size=128,
                                                    lib=lib, vals_hash=vh, verify_commits=verify)
            got = chains.blocksync_replay_dynamic(None, state, blocks, records, window=window, part_size=128, lib=lib,
                                                  verify_commits=verify,
                                                  set_hashes=lambda sets: [_valset_hash(v) for v in sets])
            assert got[:2] == want, name


def test_replay_goes_on_from_state_after(lib, fake, scenarios, wanted):
    """The state returned after a blocks is the state to replay the rest from,
    also where a change is under way: at a = 4 NextValidators differs from
    Validators, so a change takes effect on the first block of the only window."""
    state, blocks, records = scenarios["clean"]
    for a in (4, 5, 11, 14):
        head = run(lib, fake, state, blocks[:a + 1], records, 600, 1)
        assert head[:2] == (a, None)
        if a == 4:
            assert _valset_hash(head[2].next_validators) != _valset_hash(head[2].validators)
        tail = run(lib, fake, head[2], blocks[a:], records[a:], 600, 1)
        assert tail[:2] == (23 - a, None)
        assert C.same_state(C.state_dict(tail[2]), wanted["clean"][2])


def test_windows_store_nothing_on_the_shared_checks(lib, fake, scenarios, wanted, monkeypatch):
    """Windows run on several threads over one _DynamicChecks: once it is built,
    a window may read it and must not write it (only the consumer, on the
    caller's thread, records the last applied block)."""
    built = []
    init = chains._DynamicChecks.__init__

    def frozen_init(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self)

    def setattr_(self, name, value):
        assert self not in built or name == "last_applied", "a window wrote %s" % name
        object.__setattr__(self, name, value)
    monkeypatch.setattr(chains._DynamicChecks, "__init__", frozen_init)
    monkeypatch.setattr(chains._DynamicChecks, "__setattr__", setattr_, raising=False)
    for name in ("clean", "removed_proposer", "stale_validators_hash"):
        state, blocks, records = scenarios[name]
        assert same(run(lib, fake, state, blocks, records, 2, 2), wanted[name]), name


def test_a_panic_waits_for_its_block(lib, fake, scenarios, wanted):
    """The schedule is built before the first window: a change set on which the
    reference panics is raised only when the replay reaches its block, and an
    earlier block that fails ends the replay with its own error."""
    big = [(v.key_kind, v.pub_key, 1 << 59) for v in scenarios["clean"][0].validators.validators[:2]]
    for name in ("clean", "stale_next_validators_hash"):  # the latter ends at height 5
        state, blocks, records = scenarios[name]
        records = C._replace(records, 8, validator_updates=big + [C.update("e9", 1 << 59)])
        # record 8 asks for more than MaxTotalVotingPower: an error of block 9, whatever the windows
        got = run(lib, fake, state, blocks, records, 5, 2)
        if name == "clean":
            assert got[:2] == (8, (9, "commit failed for application: changing validator set: total voting power of "
                                      "resulting valset exceeds max %d" % (((1 << 63) - 1) // 8)))
        else:
            assert got[:2] == wanted[name][:2]
    # a state whose NextValidators cannot rotate (total power above MaxTotalVotingPower): the first block's
    # header names another NextValidatorsHash, an ordinary error, and the panic of its transition never comes up
    state, blocks, records = scenarios["clean"]
    heavy = [dataclasses.replace(v, voting_power=(1 << 60)) for v in state.validators.validators]
    st = dataclasses.replace(state, next_validators=H.ValidatorSet(heavy, 0))
    got = run(lib, fake, st, blocks, records, 5, 2)
    assert got[0] == 0 and got[1][0] == 1 and got[1][1].startswith("wrong Block.Header.NextValidatorsHash")


def test_panic_is_raised(lib, fake, scenarios):
    """Where the reference panics in a block's transition (a set above
    MaxTotalVotingPower cannot rotate) the driver raises, once that block's own
    checks have passed: here with set hashes that agree with the headers."""
    state, blocks, records = scenarios["clean"]
    big = [dataclasses.replace(v, voting_power=(1 << 60)) for v in state.validators.validators]
    st = dataclasses.replace(state, next_validators=H.ValidatorSet(big, 0))
    agree = blocks[0].header.validators_hash  # the genesis sets: Validators and NextValidators hash alike

    def replay(s):
        return chains.blocksync_replay_dynamic(None, s, blocks, records, window=5, depth=2, part_size=C.PART_SIZE, lib=lib,
                                               verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs),
                                               set_hashes=lambda sets: [agree] * len(sets))
    with pytest.raises(H.ValidatorSetPanic, match="Total voting power should be guarded"):
        replay(st)
    # under a first block that fails a check of its own: that error, no panic
    got = replay(dataclasses.replace(st, app_hash=b"\x01" * 32))
    assert got[0] == 0 and got[1][0] == 1 and got[1][1].startswith("wrong Block.Header.AppHash")


def test_replay_needs_a_record_per_applied_block(lib, scenarios):
    state, blocks, records = scenarios["clean"]
    with pytest.raises(ValueError, match="records"):
        chains.blocksync_replay_dynamic(None, state, blocks, records[:5], verify_commits=lambda jobs: [], lib=lib,
                                        set_hashes=lambda sets: [])
