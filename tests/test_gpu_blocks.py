"""Commit.Hash, Block.ValidateBasic and blocksync_replay_full on the device:
tmv_commit_hashes (k_commit_leaves + k_merkle_tree), the host layer's device
path and the driver against the restatement of the reference
(tests/commit_hash_ref.py).  The CPU twin is tests/test_blocks_host.py."""
import contextlib
import random

import numpy as np
import pytest

import blocks_cases as C
import commit_hash_ref as R
import merkle_ref as M
from tendermint_amd import chains, host as H
from tendermint_amd._native import NativeError
from tendermint_amd.testing.blocks import make_full_chain

pytestmark = pytest.mark.gpu


TIMED = ("k_commit_leaves", "k_merkle_leaves_long", "k_merkle_leaves", "k_merkle_tree_levels", "k_merkle_aunts")


@contextlib.contextmanager
def _launch_counts(ctx):
    """Kernel timing on inside the block (the launch counts tell which path a
    call took); nothing recorded is left behind for later tests."""
    ctx.kernel_timing(True)
    try:
        ctx.kernel_timing_read("k_commit_leaves")
        yield lambda: ctx.kernel_timing_read("k_commit_leaves")[1]
    finally:
        ctx.kernel_timing(False)
        for k in TIMED:
            ctx.kernel_timing_read(k)


def _hashes(ctx, commits):
    return [bytes(r) for r in ctx.commit_hashes(*C.columns(commits))]


def _want(commits):
    return [R.commit_hash_of_sigs(c) for c in commits]


def test_commit_hashes_every_size_and_encoder_case(ctx):
    """One launch: commits of 0 .. 257 signatures, every encoder case, an
    empty commit in the middle (largest commit 257: the 256-lane tree kernel)."""
    C.check_case_lengths()
    rng = random.Random(1)
    commits = [[C.random_sig(rng) for _ in range(n)] for n in (0, 1, 2, 3, 64, 65, 128, 129, 257)]
    commits.insert(5, [])
    commits.append(list(C.ENCODER_CASES.values()))
    commits.append(list(C.OUT_OF_DOMAIN_CASES.values()))
    for case in list(C.ENCODER_CASES.values()) + list(C.OUT_OF_DOMAIN_CASES.values()):
        commits.append([case])  # each case as a commit of its own: the leaf is the root
    got = _hashes(ctx, commits)
    assert got == _want(commits)
    assert got[0] == got[5] == M.empty_hash()


@pytest.mark.parametrize("largest", [128, 129])
def test_commit_hashes_both_tree_kernels(ctx, largest):
    """At most 128 signatures per commit: one wave per tree; above: 256 lanes."""
    rng = random.Random(largest)
    commits = [[C.random_sig(rng) for _ in range(n)] for n in (5, largest, 0, 17, 127)]
    assert _hashes(ctx, commits) == _want(commits)


def test_commit_hashes_argument_errors(ctx):
    good = [[C.ENCODER_CASES["flag2"], C.ENCODER_CASES["absent"]], [C.ENCODER_CASES["sig1"]]]
    flag, alen, addr, secs, nanos, slen, sig, off = C.columns(good)
    assert [bytes(r) for r in ctx.commit_hashes(flag, alen, addr, secs, nanos, slen, sig, off)] == _want(good)

    def bad(**kw):
        a = dict(flag=flag.copy(), alen=alen.copy(), slen=slen.copy(), off=off.copy())
        for name, (i, v) in kw.items():
            a[name][i] = v
        with pytest.raises(NativeError, match=r"\(-1\)"):
            ctx.commit_hashes(a["flag"], a["alen"], addr, secs, nanos, a["slen"], sig, a["off"])
    bad(flag=(1, 128))
    bad(alen=(0, 19))
    bad(slen=(2, 65))
    bad(off=(0, 1))   # commit_off[0] != 0
    with pytest.raises(NativeError, match=r"\(-1\)"):
        ctx.commit_hashes(flag, alen, addr, secs, nanos, slen, sig, np.array([0, 3, 2], np.uint32))
    # a zero-commit call
    z8 = np.zeros(0, np.uint8)
    assert len(ctx.commit_hashes(z8, z8, z8, np.zeros(0, np.int64), np.zeros(0, np.int32), z8, z8,
                                 np.zeros(1, np.uint32))) == 0


def test_host_commit_hashes_device_and_host_paths_agree(ctx):
    """40 commits take the device path (at least 32 per call), 5 the host's;
    a commit with a 19-byte address is refused by the engine and hashed on the
    host inside the device call."""
    rng = random.Random(9)
    sigs = [[C.random_sig(rng) for _ in range(7)] for _ in range(40)]
    sigs[11][3] = (2, C.ADDR[:19], C.T, 1, C.SIG)
    commits = [C.host_commit(s) for s in sigs]
    want = _want(sigs)
    with _launch_counts(ctx) as launches:
        got = H.commit_hashes(ctx, commits)
        assert launches() == 1
        assert got == want
        for lo in range(0, 40, 5):
            assert H.commit_hashes(ctx, commits[lo:lo + 5]) == want[lo:lo + 5]
        assert launches() == 0
    assert H.commit_hashes(ctx, commits[:3] + [None] + commits[3:]) == want[:3] + [None] + want[3:]


def test_blocks_validate_basic_window(ctx):
    C.check_validate_basic(ctx, None, C.window_blocks(40))


def test_blocks_validate_basic_below_the_threshold_is_the_same(ctx):
    blocks = C.window_blocks(40)
    want = [(R.block_validate_basic(b), R.block_hash(b)) for b in blocks]
    with _launch_counts(ctx) as launches:
        assert H.blocks_validate_basic(ctx, blocks[:7]) == want[:7]
        assert launches() == 0
        assert H.blocks_validate_basic(ctx, blocks) == want
        assert launches() == 1


@pytest.fixture(scope="module")
def chain():
    vals, blocks, ids = make_full_chain(40, 5, C.CHAIN, seed=43, raw_len=(1, 200000), txs=(0, 5))
    return vals, blocks, ids, C.SigCache()


def test_blocksync_replay_full_clean_and_tampered(ctx, chain):
    vals, blocks, ids, cache = chain
    assert chains.validator_set_hashes(ctx, [vals])[0] == blocks[0].header.validators_hash

    def run(bl, last, height):
        return chains.blocksync_replay_full(ctx, C.CHAIN, vals, bl, last, window=16, last_block_height=height)
    C.check_replay(run, cache, vals, blocks, ids, 23, names=("clean", "tx_tampered"))
    assert run(blocks, H.BlockID(), 0) == (39, None)


def test_blocksync_replay_full_one_window(ctx, chain):
    vals, blocks, ids, cache = chain

    def run(bl, last, height):
        return chains.blocksync_replay_full(ctx, C.CHAIN, vals, bl, last, last_block_height=height)
    C.check_replay(run, cache, vals, blocks, ids, 30,
                   names=("commit_sig_time_tampered", "wrong_last_block_id", "wrong_raw_length"))
