"""chains.blocksync_replay_dynamic on the engine: the chain of
tests/valset_chain_cases.py with the signatures verified and the set hashes,
header hashes and result roots computed by libtmgpu.so, against the CPU build
of the host layer (tests/test_replay_dynamic.py runs the same there)."""
import ctypes
import os

import pytest

import commit_fixtures as F
import valset_chain_cases as C
from tendermint_amd import chains, host as H
from tendermint_amd.testing.factory import _valset_hash

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libvalsethost.so")


@pytest.fixture(scope="module")
def scenarios():
    return C.scenarios()


@pytest.fixture(scope="module")
def cpu():
    """blocksync_replay_dynamic on the CPU build: no engine, the C oracle's signature checks."""
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(LIB)
    fake = F.FakeBackend()
    fake.real_signatures(True)

    def run(state, blocks, records):
        return chains.blocksync_replay_dynamic(None, state, blocks, records, window=5, part_size=C.PART_SIZE, lib=lib,
                                               verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs),
                                               set_hashes=lambda sets: [_valset_hash(vs) for vs in sets])
    yield run
    fake.real_signatures(False)


def on_engine(ctx, state, blocks, records, wire=False, **kw):
    return chains.blocksync_replay_dynamic(ctx, state, [b.raw for b in blocks] if wire else blocks, records, window=5,
                                           part_size=C.PART_SIZE, wire=wire, **kw)


def same(got, want):
    return got[:2] == want[:2] and C.same_state(C.state_dict(got[2]), C.state_dict(want[2]))


@pytest.mark.parametrize("wire", [False, True])
def test_the_chain_on_the_engine(ctx, cpu, scenarios, wire):
    state, blocks, records = scenarios["clean"]
    want = cpu(state, blocks, records)
    assert want[:2] == (23, None)
    got = on_engine(ctx, state, blocks, records, wire)
    assert same(got, want)
    # a second replay on the same context: the key caches hold the keys by now
    assert same(on_engine(ctx, state, blocks, records, wire), want)


@pytest.mark.parametrize("wire", [False, True])
def test_wrong_chains_on_the_engine(ctx, cpu, scenarios, wire):
    """A tampered signature in a commit around a change of the set, a commit
    that the set from before the change signed, a signature of the other key
    type, a stale hash, a failed transition."""
    for name in ("tampered_signature", "signed_by_the_old_set", "other_key_signs", "stale_validators_hash",
                 "unknown_removal"):
        state, blocks, records = scenarios[name]
        want = cpu(state, blocks, records)
        assert want[1] is not None, name
        assert same(on_engine(ctx, state, blocks, records, wire), want), name


def test_a_secp256k1_validator_joins(ctx, monkeypatch):
    """The mixed set is hashed by the host layer, the others in the window's one
    device call; the verdicts equal the one-at-a-time loop on the engine."""
    state, blocks, records = C.scenarios("k0")["clean"]
    want = C.replay_one_at_a_time(F.GpuBackend(ctx), state, blocks, records)
    assert want[:2] == (23, None)
    on_host, device_calls = [], []
    host_hash, device_hashes = H.validator_set_hash_host, chains.validator_set_hashes

    def count_host(vs, lib=None):
        on_host.append(vs)
        return host_hash(vs, lib)

    def count_device(c, sets):
        device_calls.append(len(sets))
        return device_hashes(c, sets)
    monkeypatch.setattr(H, "validator_set_hash_host", count_host)
    monkeypatch.setattr(chains, "validator_set_hashes", count_device)
    got = on_engine(ctx, state, blocks, records)
    assert got[:2] == want[:2] and C.same_state(C.state_dict(got[2]), want[2])
    assert on_host and all(any(v.key_kind == H.TMV_KIND_SECP256K1 for v in vs.validators) for vs in on_host)
    # at most one device call per window of 5 over 23 blocks, none for a window whose sets all hold the key
    assert 1 <= len(device_calls) <= 5 and all(n > 0 for n in device_calls)
    for vs in on_host:
        assert host_hash(vs) == _valset_hash(vs)
