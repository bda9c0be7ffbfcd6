"""Split key scalars in the batch equation (tendermint_amd/csrc/split.h): a
group with at most split_max leaders (distinct live keys after run merging)
relabels the high windows of its A and B scalars onto high points, so that it
fills half the windows.  The group sum is the same group element, so every
vector below must equal the C oracle's batch by batch, with the path forced on
(test aid split_groups = 1; it starts at 2,048 groups in the product) and at
its default (off at these sizes: no group splits).  The device's counts of
split groups and of high points computed (tmv_split_stats) must equal the
counts computed here from the slot order, the key encodings and
ed25519_prechecks; with the located pass on, the failing and located group
counts must be those the slot order predicts."""
import numpy as np
import pytest

import oracle_c as C
from tendermint_amd import _native as N
from test_gpu_key_runs import (SEED, _option, bad_launch, commit, expected_groups, flip_s, launch, oracle,
                               slot_order)

pytestmark = pytest.mark.gpu

SPLIT_MAX = 8  # msm.h kMsmSplitMax


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = N.Context(1)
    yield c
    c.close()
    _option(b"split_groups", 0)
    _option(b"split_max", 0)


_live = {}


def live_mask(b):
    key = (b.pk.tobytes(), b.sig.tobytes())
    if key not in _live:
        _live[key] = C.ed25519_prechecks(b.pk, b.sig).astype(bool) if b.n else np.zeros(0, bool)
    return _live[key]


def expected_split(batches, m, split_max):
    """(split groups, high points) of the launch in column order: a group's
    leaders are the distinct key encodings among its live entries."""
    live = [live_mask(b) for b in batches]
    order = slot_order([b.n for b in batches], 64)
    groups = points = 0
    for g in range(0, len(order), m):
        keys = {batches[j].pk[32 * i:32 * i + 32].tobytes() for j, i in order[g:g + m] if live[j][i]}
        if len(keys) <= split_max:
            groups += 1
            points += len(keys)
    return groups, points


def check(ctx, batches, shifts=None, group_log2s=(6, 7), located=False, split_max=SPLIT_MAX):
    """The launch with the split forced on and at its default, groups of 64
    and 128: the oracle's vectors, and the device's split counts."""
    want = [oracle(b) for b in batches]
    seen = []
    try:
        for m_log2 in group_log2s:
            ctx.set_batch_options(group_log2=m_log2, seed=SEED, stats=True)
            for forced in (1, 0):
                _option(b"split_groups", forced)
                s0, f0 = ctx.split_stats(), ctx.group_fail_stats()
                got = launch(ctx, batches, shifts)
                s1, f1 = ctx.split_stats(), ctx.group_fail_stats()
                where = (m_log2, forced)
                for k, (g, w) in enumerate(zip(got, want)):
                    assert np.array_equal(g, w), (where, k, np.flatnonzero(g != w)[:8])
                exp = expected_split(batches, 1 << m_log2, split_max) if forced else (0, 0)
                have = (s1["groups_split"] - s0["groups_split"], s1["high_points"] - s0["high_points"])
                print(where, "split groups, high points", have, "expected", exp)
                assert have == exp, where
                failed, single = expected_groups(batches, 64, 1 << m_log2)
                assert f1["failed"] - f0["failed"] == failed, where
                assert f1["located"] - f0["located"] == (single if located else 0), where
                if forced:
                    seen.append(have)
    finally:
        _option(b"split_groups", 0)
    return want, seen


@pytest.mark.parametrize("K", [64, 8, 4, 1, 65, 130])
def test_honest_shapes(ctx, K):
    """65 validators.  64 batches: one leader per group of 64; 8: exactly
    split_max; 4: 16 leaders, no group splits; 1: no runs; 65 and 130: a second
    tile that merges nothing (65) or a full tile, a full tile and a pair, so
    one launch mixes split and unsplit groups."""
    batches = [commit(65, 10 + j % 64) for j in range(K)]
    want, seen = check(ctx, batches)
    assert all(w.all() for w in want)
    groups64 = -(-65 * K // 64)
    if K == 64:
        assert seen[0] == (65, 65)  # groups of 64: a column each
    if K == 8:
        assert seen[0] == (groups64, 65)  # 8 columns a group, the last group one
    if K in (4, 1):
        assert seen[0] == (1, 1)  # only the last group, which holds one column (K = 4) or one entry
    if K in (65, 130):
        assert 0 < seen[0][0] < groups64


def test_ragged_launch(ctx):
    """test_gpu_key_runs.test_ragged_launch's launch: keys shift between
    columns, one empty batch, one at an unaligned address."""
    rng = np.random.default_rng(3)
    batches = []
    for j in range(70):
        b = commit(65, 10 + j % 64)
        if j % 3 == 1:
            b = b.take(np.sort(rng.choice(65, 65 - 1 - j % 7, replace=False)))
        if j == 4:
            b = b.take([])
        if j == 6:
            b = flip_s(b, [2])
        batches.append(b)
    check(ctx, batches, shifts={2: 3, 9: 1})


@pytest.mark.parametrize("K", [2, 64, 65])
def test_bad_entries(ctx, K):
    """A leader whose own signature is bad, a leader whose key does not
    decode, a dead column, small-order and non-canonical key columns (their
    high points go through torsion and the identity), two bad in one group."""
    check(ctx, bad_launch(K))


@pytest.mark.parametrize("K", [2, 64, 65])
def test_bad_entries_located(ctx, K, monkeypatch):
    """The same with the located pass on: its sort takes the primary pass's
    split decisions and high points."""
    monkeypatch.setenv("TMV_LOCATE_MIN", "1")
    check(ctx, bad_launch(K), located=True)


def test_same_batch_twice(ctx, monkeypatch):
    a, b = flip_s(commit(65, 10), [4]), flip_s(commit(65, 11), [40])
    check(ctx, [a, b, a, b, commit(65, 12), a])
    monkeypatch.setenv("TMV_LOCATE_MIN", "1")
    check(ctx, [a, b, a, b, commit(65, 12), a], located=True)


def test_threshold_of_one(ctx):
    """split_max = 1: only the groups that hold a single key split (64
    batches, groups of 64: every full column; groups of 128 hold two)."""
    _option(b"split_max", 1)
    try:
        want, seen = check(ctx, [commit(65, 10 + j) for j in range(64)], split_max=1)
    finally:
        _option(b"split_max", 0)
    assert seen[0][0] > 0 and seen[1][0] <= 1
