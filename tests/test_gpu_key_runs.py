"""Runs of one key in the batch equation (msm.h, colorder.h): multi-batch
ed25519 launches order their work slots down the columns of tiles of 64
batches, and k_msm_sort folds the A terms of entries that share a key
encoding inside a group into one scalar.  Every vector below must equal the C
oracle's batch by batch, with the column order on and off, for groups of 64
and 128, with bad entries wherever a run's bookkeeping could go wrong; the
point cache must still serve the permuted launch; and the device's count of
bucket entries must show that runs really merged.  Every launch's count of
failing groups (tmv_group_fail_stats, counted on the device) must equal the
count computed here from the slot order and the oracle vector, and with the
located pass on, the groups it names must be the failing groups with exactly
one bad entry.  Every launch also runs with run merging switched off and with
k_msm_accum's compact lane order forced on (it starts at 2,048 groups in the
product)."""
import ctypes
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_c as C
from tendermint_amd import _native as N
from tendermint_amd.testing.factory import Batch, make_commit_batch, undecodable_encodings

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ED, BEQ = N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_ORDER = 2**252 + 27742317777372353535851937790883648493


def _option(name, v):
    L = N.lib()
    L.tmv_internal_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    assert L.tmv_internal_option(name, int(v)) == 0


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = N.Context(1)
    yield c
    c.close()
    _option(b"column_tile", -1)
    _option(b"key_merge", 1)
    _option(b"compact_groups", 0)
    _option(b"point_cache_min", 0)


_commits = {}


def commit(n_vals, h):
    """make_commit_batch(n_vals, height=h): the same keys in the same order, distinct messages."""
    if (n_vals, h) not in _commits:
        _commits[(n_vals, h)] = make_commit_batch(n_vals, height=h)
    return _commits[(n_vals, h)]


def with_sig(b, sig):
    return Batch(b.pk, sig, b.msg, b.off, b.kinds)


def flip_s(b, entries):
    """One low S bit of each entry flipped (S stays canonical, the equation fails)."""
    sig = b.sig.copy()
    for i in entries:
        sig[64 * i + 32] ^= 1
    return with_sig(b, sig)


_oracle = {}


def oracle(b):
    key = (b.pk.tobytes(), b.sig.tobytes(), b.msg.tobytes())
    if key not in _oracle:
        _oracle[key] = C.ed25519_verify_packed(b.pk, b.sig, b.msg, b.off, threads=8)[1] if b.n else np.zeros(0, np.uint8)
    return _oracle[key]


def launch(ctx, batches, shifts=None):
    """One tmv_verify_batches_device launch; the batches' status vectors."""
    import torch
    dev = torch.device("cuda:0")
    keep, refs, outs = [], [], []
    for k, b in enumerate(batches):
        if b.n == 0:
            refs.append(N.BatchRef(0, 0, 0, 0, 0, 0, 0))
            outs.append(None)
            continue
        shift = shifts.get(k, 0) if shifts else 0
        raw = {}
        for f in ("pk", "sig", "msg"):
            a = getattr(b, f)
            buf = torch.zeros(len(a) + 16, dtype=torch.uint8, device=dev)
            buf[shift:shift + len(a)] = torch.from_numpy(a).to(dev)
            raw[f] = buf
        off = torch.from_numpy(b.off.view(np.int32)).to(dev)
        out = torch.full((b.n,), -7, dtype=torch.int8, device=dev)
        keep += [raw, off, out]
        refs.append(N.BatchRef(raw["pk"].data_ptr() + shift, raw["sig"].data_ptr() + shift,
                               raw["msg"].data_ptr() + shift, off.data_ptr(), b.n, int(b.off[-1] - b.off[0]),
                               out.data_ptr()))
        outs.append(out)
    torch.cuda.synchronize()
    ctx.verify_batches_device(0, ED, BEQ, refs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy().astype(np.uint8) if o is not None else np.zeros(0, np.uint8) for o in outs]


_pre = {}


def bad_mask(b):
    """Entries the batch equation includes (pre-checks pass) that are invalid: each fails its group."""
    key = (b.pk.tobytes(), b.sig.tobytes(), b.msg.tobytes())
    if key not in _pre:
        _pre[key] = (C.ed25519_prechecks(b.pk, b.sig) & (oracle(b) == 0)) if b.n else np.zeros(0, bool)
    return _pre[key]


def slot_order(counts, T):
    """(batch, entry) of every work slot: batch order for T = 0 or one batch,
    else row by row inside tiles of T batches (colorder.h, restated)."""
    K = len(counts)
    if T == 0 or K <= 1:
        return [(j, i) for j in range(K) for i in range(counts[j])]
    order = []
    for t0 in range(0, K, T):
        tile = range(t0, min(t0 + T, K))
        for i in range(max(counts[j] for j in tile)):
            order += [(j, i) for j in tile if counts[j] > i]
    return order


def expected_groups(batches, T, m):
    """(failing groups, failing groups with exactly one bad entry) of the launch."""
    masks = [bad_mask(b) for b in batches]
    bad = np.array([masks[j][i] for j, i in slot_order([b.n for b in batches], T)], bool)
    per = [int(bad[g:g + m].sum()) for g in range(0, len(bad), m)]
    return sum(c > 0 for c in per), sum(c == 1 for c in per)


# (column tile, run merging, compact_groups): the product; batch order; the
# column order without merging; both orders with the accumulation's compact
# lane order forced on at any group count
LEGS = [(-1, 1, 0), (0, 1, 0), (-1, 0, 0), (-1, 1, 1), (0, 1, 1)]


def check(ctx, batches, shifts=None, group_log2s=(6, 7), located=False):
    """The launch on every leg, groups of 64 and 128: every batch's vector
    equals the oracle's (so all legs give identical vectors), and the device
    counted the failing (and located) groups the slot order predicts."""
    want = [oracle(b) for b in batches]
    try:
        for m_log2 in group_log2s:
            ctx.set_batch_options(group_log2=m_log2, seed=SEED, stats=True)
            for tile, merge, compact in LEGS:
                _option(b"column_tile", tile)
                _option(b"key_merge", merge)
                _option(b"compact_groups", compact)
                s0 = ctx.group_fail_stats()
                got = launch(ctx, batches, shifts)
                s1 = ctx.group_fail_stats()
                where = (m_log2, tile, merge, compact)
                for k, (g, w) in enumerate(zip(got, want)):
                    assert np.array_equal(g, w), (where, k, np.flatnonzero(g != w)[:8])
                failed, single = expected_groups(batches, 64 if tile else 0, 1 << m_log2)
                print(where, "failed", s1["failed"] - s0["failed"], "expected", failed,
                      "located", s1["located"] - s0["located"], "expected", single if located else 0)
                assert s1["failed"] - s0["failed"] == failed, where
                assert s1["located"] - s0["located"] == (single if located else 0), where
    finally:
        _option(b"column_tile", -1)
        _option(b"key_merge", 1)
        _option(b"compact_groups", 0)
    return want


@pytest.mark.parametrize("n_vals", [1, 31, 65, 257])
@pytest.mark.parametrize("K", [1, 2, 64, 65, 130])
def test_honest_shapes(ctx, K, n_vals):
    """Every size at which the order or the runs change shape: one batch (no
    permutation), a tile of two, a full tile, a second tile of one batch that
    merges nothing, two tiles and a part; one key, less than a group, just
    over a group of 64, just over two groups of 128."""
    want = check(ctx, [commit(n_vals, 10 + j) for j in range(K)])
    assert all(w.all() for w in want)


def bad_launch(K=64, n_vals=65):
    """K commits with, in separate columns: one bad S bit, two bad in one
    group, a whole bad column, the run leader's own signature bad, the
    leader's key undecodable, columns of small-order / non-canonical keys, and
    a column whose keys are all undecodable (with 64 batches and groups of 64,
    a group whose entries are all dead)."""
    g = json.load(open(os.path.join(REPO, "tests", "golden", "zip215_small_order.json")))
    enc = [bytes.fromhex(e) for e in g["encodings"]]
    undec = undecodable_encodings(3, random.Random(9))
    out = []
    for j in range(K):
        b = commit(n_vals, 10 + j)
        bad = [11]                                   # a whole bad column
        if j == 5 % K:
            bad += [3, 7]                            # one bad entry in column 3; first of two in column 7
        if j == 9 % K:
            bad += [7]
        if j == 0:
            bad += [13]                              # the run leader's own signature
        b = flip_s(b, sorted(set(bad)))
        pk, sig = b.pk.copy(), b.sig.copy()
        if j == 0:
            pk[32 * 17:32 * 18] = np.frombuffer(undec[0], np.uint8)   # the leader's key does not decode
        if j == 1 % K:
            pk[32 * 18:32 * 19] = np.frombuffer(undec[1], np.uint8)   # an absent validator inside a run
        for col, e in ((19, 0), (20, len(enc) // 2), (21, len(enc) - 1)):  # torsion under a merged scalar
            pk[32 * col:32 * col + 32] = np.frombuffer(enc[e], np.uint8)
            sig[64 * col:64 * col + 32] = np.frombuffer(enc[(e + 1 + j) % len(enc)], np.uint8)
            sig[64 * col + 32:64 * col + 64] = 0
        pk[32 * 23:32 * 24] = np.frombuffer(undec[2], np.uint8)       # a dead column
        out.append(Batch(pk, sig, b.msg, b.off, b.kinds))
    return out


@pytest.mark.parametrize("K", [2, 64, 65])
def test_bad_entries(ctx, K):
    want = check(ctx, bad_launch(K))
    assert not want[0][11] and not want[0][13] and not want[0][17] and want[0][19] and want[0][12]
    assert not any(w[23] for w in want)


@pytest.mark.parametrize("K", [2, 64, 65])
def test_bad_entries_located(ctx, K, monkeypatch):
    """The same launches with the located pass on (its second, index-weighted
    sort merges runs too)."""
    monkeypatch.setenv("TMV_LOCATE_MIN", "1")
    check(ctx, bad_launch(K), located=True)


def test_same_batch_twice(ctx, monkeypatch):
    """The benchmark's situation: a launch lists one batch more than once, so
    a bad signature sits twice in its group."""
    a, b = flip_s(commit(65, 10), [4]), flip_s(commit(65, 11), [40])
    check(ctx, [a, b, a, b, commit(65, 12), a])
    monkeypatch.setenv("TMV_LOCATE_MIN", "1")
    check(ctx, [a, b, a, b, commit(65, 12), a], located=True)


def test_ragged_launch(ctx):
    """Batches with entries removed, so that keys shift between columns; one
    empty batch; one at an unaligned address."""
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


def test_ragged_launch_located(ctx, monkeypatch):
    """A ragged launch with bad entries under the located pass: the slot
    function alone says which groups they fall into."""
    monkeypatch.setenv("TMV_LOCATE_MIN", "1")
    rng = np.random.default_rng(4)
    batches = []
    for j in range(66):
        b = commit(65, 10 + j % 64)
        if j % 4 == 2:
            b = b.take(np.sort(rng.choice(65, 65 - 1 - j % 5, replace=False)))
        if j == 7:
            b = b.take([])
        if j in (3, 20, 21, 65):
            b = flip_s(b, [5, b.n - 1] if j != 21 else [5])
        batches.append(b)
    check(ctx, batches, located=True)


def test_point_cache_with_the_permutation(ctx, monkeypatch):
    """Cold, then warm: both vectors exact, and the second launch's hits are
    the entries whose key decodes."""
    from test_gpu_point_cache import _no_shared_slot
    monkeypatch.setenv("TMV_POINT_CACHE_SLOTS", str(1 << 21))
    _option(b"point_cache_min", 512)
    c = N.Context(1)
    try:
        batches = bad_launch(64)
        want = [oracle(b) for b in batches]
        keys = [b.pk[32 * i:32 * i + 32].tobytes() for b in batches for i in range(b.n)]
        # every R of these launches decodes and every S is canonical: the pre-checks are A's decode
        a_ok = np.concatenate([C.ed25519_prechecks(b.pk, b.sig) for b in batches])
        case = SimpleNamespace(keys=keys, decodable=a_ok)
        assert _no_shared_slot(case, 1 << 21)
        c.set_batch_options(group_log2=7, seed=SEED, stats=True)
        n = len(keys)
        s0 = c.point_cache_stats()
        for w, g in zip(want, launch(c, batches)):
            assert np.array_equal(g, w)
        s1 = c.point_cache_stats()
        assert s1["hits"] + s1["misses"] - s0["hits"] - s0["misses"] == n
        for w, g in zip(want, launch(c, batches)):
            assert np.array_equal(g, w)
        s2 = c.point_cache_stats()
        assert (s2["hits"] - s1["hits"], s2["misses"] - s1["misses"]) == (int(a_ok.sum()), n - int(a_ok.sum()))
    finally:
        c.close()
        _option(b"point_cache_min", 0)


def digit_counts(c=5, samples=4000, seed=1):
    """Mean nonzero signed c-bit digits of a 128-bit weight (R term) and of a
    scalar mod l (A or B term): k_msm_sort's recoding, restated."""
    rng = random.Random(seed)

    def nonzero(x, windows):
        cnt, carry = 0, 0
        for w in range(windows):
            d = ((x >> (w * c)) & ((1 << c) - 1)) + carry
            if w + 1 < windows and d >= 1 << (c - 1):
                d -= 1 << c
                carry = 1
            else:
                carry = 0
            cnt += d != 0
        return cnt
    wr, w = -(-129 // c), -(-254 // c)
    r = sum(nonzero(rng.getrandbits(128), wr) for _ in range(samples)) / samples
    a = sum(nonzero(rng.randrange(L_ORDER), w) for _ in range(samples)) / samples
    return r, a


@pytest.mark.parametrize("m_log2", [6, 7])
def test_entry_counter(ctx, m_log2):
    """64 equal batches of honest keys: a group of m holds m / 64 runs, so a
    signature costs its R digits plus (runs + 1) / m of an A-sized term;
    with the order off, or with the order on and merging off, it costs what
    it always did.  Within 2 %."""
    K, n_vals, m = 64, 256, 1 << m_log2
    batches = [commit(n_vals, 10 + j) for j in range(K)]
    r, a = digit_counts(c=5)
    per_sig = {}
    for tile, merge in ((-1, 1), (0, 1), (-1, 0)):
        _option(b"column_tile", tile)
        _option(b"key_merge", merge)
        ctx.set_batch_options(group_log2=m_log2, window_bits=5, seed=SEED, stats=True)
        e0 = ctx.bucket_entry_stats()
        got = launch(ctx, batches)
        per_sig[(tile, merge)] = (ctx.bucket_entry_stats() - e0) / (K * n_vals)
        assert all(g.all() for g in got)
    _option(b"column_tile", -1)
    _option(b"key_merge", 1)
    print(f"entries per signature, m = {m}: merged {per_sig[(-1, 1)]:.2f}, batch order {per_sig[(0, 1)]:.2f}, "
          f"column order without merging {per_sig[(-1, 0)]:.2f}")
    merged = r + a * (m // 64 + 1) / m
    plain = r + a + a / m
    assert abs(per_sig[(-1, 1)] - merged) <= 0.02 * merged, (per_sig, merged)
    assert abs(per_sig[(0, 1)] - plain) <= 0.02 * plain, (per_sig, plain)
    assert abs(per_sig[(-1, 0)] - plain) <= 0.02 * plain, (per_sig, plain)
