"""The hash of ABCI results on the device: tmv_tx_results_hashes
(k_result_leaves + k_merkle_tree), the host layer's device path and
blocksync_replay_stateful on the engine, every launch bit for bit against the
restatement of the reference (tests/results_ref.py).  The CPU twin is
tests/test_results_host.py."""
import contextlib
import random

import numpy as np
import pytest

import merkle_ref as M
import results_cases as C
import results_ref as R
from tendermint_amd import chains, host as H
from tendermint_amd._native import NativeError

pytestmark = pytest.mark.gpu

TIMED = ("k_result_leaves", "k_merkle_leaves", "k_merkle_leaves_long")


@contextlib.contextmanager
def _launch_counts(ctx):
    """Kernel timing on inside the block (the launch counts tell which path a
    call took); nothing recorded is left behind for later tests."""
    ctx.kernel_timing(True)
    try:
        for k in TIMED:
            ctx.kernel_timing_read(k)
        yield lambda k="k_result_leaves": ctx.kernel_timing_read(k)[1]
    finally:
        ctx.kernel_timing(False)
        for k in TIMED:
            ctx.kernel_timing_read(k)


def _roots(ctx, trees, firsts=None):
    extra = C.first_columns(firsts) if firsts is not None else ()
    return [bytes(r) for r in ctx.tx_results_hashes(*C.columns(trees), *extra)]


def _want(trees, firsts=None):
    return [R.results_hash(t, firsts[k] if firsts is not None else None) for k, t in enumerate(trees)]


def test_whole_case_table_in_one_launch(ctx):
    """Every encoder case as a tree of its own (the leaf is the root), the
    table as one tree, trees of every size class, empty trees between them."""
    C.check_case_lengths()
    cases = list(C.CASES.values())
    trees = [[c] for c in cases] + [cases, []] + [C.tree(n, 10 + n) for n in C.TREE_SIZES] + [[]]
    with _launch_counts(ctx) as launches:
        got = _roots(ctx, trees)
        assert launches() == 1
    assert got == _want(trees)
    assert got[len(cases) + 1] == got[-1] == M.empty_hash()
    assert got[0] == M.leaf_hash(b"")  # the empty result is a leaf, not an empty tree


@pytest.mark.parametrize("largest", [1, 64, 65, 128, 129])
def test_both_tree_kernels(ctx, largest):
    """At most 128 leaves per tree: one wave per tree; above: 256 lanes."""
    trees = [C.tree(n, largest + n) for n in (min(5, largest), largest, 0, min(17, largest), largest - 1)]
    assert _roots(ctx, trees) == _want(trees)
    firsts = [b"f" * k for k in range(len(trees))]  # with the leading leaf the largest tree has one more
    assert _roots(ctx, trees, firsts) == _want(trees, firsts)


def test_no_results_and_no_trees(ctx):
    trees = [[], [], []]
    assert _roots(ctx, trees) == [M.empty_hash()] * 3
    assert _roots(ctx, trees, [b"", b"x", b""]) == [M.leaf_hash(b""), M.leaf_hash(b"x"), M.leaf_hash(b"")]
    z = np.zeros(0, np.uint8)
    assert len(ctx.tx_results_hashes(z, z, z, z, np.zeros(1, np.uint32), np.zeros(1, np.uint32))) == 0
    assert len(ctx.tx_results_hashes(z, z, z, None, np.zeros(1, np.uint32), np.zeros(1, np.uint32), None,
                                     np.zeros(1, np.uint32))) == 0


def test_first_leaf(ctx):
    """Leading leaves of 0, 1, 55, 56 and 200 bytes through the byte-wise leaf
    kernel; a call whose leading leaves average above the long-leaf crossover
    (512 bytes) through k_merkle_leaves_long, an empty one among them."""
    sizes = (0, 1, 55, 56, 200, 54, 57)
    trees = [C.tree(n, 30 + n) for n in (3, 0, 1, 64, 128, 129, 2)]
    firsts = [C._data(s) for s in sizes]
    with _launch_counts(ctx) as launches:
        assert _roots(ctx, trees, firsts) == _want(trees, firsts)
        assert (launches("k_merkle_leaves"), launches("k_merkle_leaves_long"), launches()) == (1, 0, 1)
        long_firsts = [C._data(s) for s in (0, 700, 5000, 1, 513, 3000, 64)]
        assert _roots(ctx, trees, long_firsts) == _want(trees, long_firsts)
        assert (launches("k_merkle_leaves"), launches("k_merkle_leaves_long"), launches()) == (0, 1, 1)
    # without the flag first and first_off are ignored
    cols = C.columns(trees)
    got = ctx.tx_results_hashes(*cols, *C.first_columns(firsts), flags=0)
    assert [bytes(r) for r in got] == _want(trees)


def test_ragged_call(ctx):
    """300 trees of 0 to 300 results with 0 to 300 data bytes each, one result of 64 KiB."""
    rng = random.Random(2024)
    nrng = np.random.default_rng(2024)
    trees = []
    for _ in range(300):
        n = rng.randint(0, 300)
        lens = nrng.integers(0, 301, n)
        blob = nrng.bytes(int(lens.sum()))
        at = np.concatenate(([0], np.cumsum(lens)))
        trees.append([(rng.choice([0, 1, 300, 1 << 31]), blob[at[i]:at[i + 1]], rng.choice([0, 5, -1, 1 << 40]),
                       rng.choice([0, 77, C.I64_MIN])) for i in range(n)])
    trees[150].insert(len(trees[150]) // 2, (9, nrng.bytes(65536), 1, 2))
    assert _roots(ctx, trees) == _want(trees)


def test_argument_errors(ctx):
    trees = [[C.CASES["code127_data"], C.CASES["data1"], C.CASES["leaf55"]], [C.CASES["data127"], C.CASES["empty"]]]
    code, gw, gu, data, doff, toff = C.columns(trees)
    first, foff = C.first_columns([b"ab", b""])
    assert [bytes(r) for r in ctx.tx_results_hashes(code, gw, gu, data, doff, toff, first, foff)] == \
        _want(trees, [b"ab", b""])

    def bad(*a, **kw):
        with pytest.raises(NativeError, match=r"\(-1\)"):
            ctx.tx_results_hashes(*a, **kw)

    def edited(off, i, v):
        o = off.copy()
        o[i] = v
        return o
    bad(code, gw, gu, data, edited(doff, 0, 1), toff)                 # data_off[0] != 0
    bad(code, gw, gu, data, edited(doff, 2, 0), toff)                 # decreasing
    bad(code, gw, gu, data, doff, edited(toff, 0, 1))                 # tree_off[0] != 0
    bad(code, gw, gu, data, doff, np.array([0, 5, 3], np.uint32))     # decreasing
    bad(code, gw, gu, data, doff, toff, first, edited(foff, 0, 1))    # first_off[0] != 0
    bad(code, gw, gu, data, doff, toff, first, np.array([0, 2, 1], np.uint32))
    bad(code, gw, gu, data, doff, toff, flags=2)                      # an unknown flag bit
    bad(code, gw, gu, data, doff, toff, first, foff, flags=5)
    bad(code, gw, gu, None, doff, toff)                               # null data with data bytes
    bad(code, gw, gu, data, doff, toff, None, foff)                   # null first with leading-leaf bytes
    bad(code, gw, gu, data, doff, toff, first, None, flags=1)         # the flag without first_off
    bad(code, gw, gu, data, doff, np.array([0, 3, (1 << 26) + 1], np.uint32))  # more than 2^26 results


def _paths(monkeypatch, ctx, fn):
    """fn() on the device path (the knob at 1), then on the host path: (device, host, launches on the device path)."""
    with _launch_counts(ctx) as launches:
        monkeypatch.setenv("TMV_DEVICE_RESULTS_MIN", "1")
        dev = fn()
        n = launches()
        monkeypatch.setenv("TMV_DEVICE_RESULTS_MIN", str(1 << 40))
        host = fn()
        assert launches() == 0
    monkeypatch.delenv("TMV_DEVICE_RESULTS_MIN")
    return dev, host, n


@pytest.mark.parametrize("first", [False, True])
def test_host_layer_paths_agree(ctx, monkeypatch, first):
    trees = [C.tree(n, 70 + n) for n in C.TREE_SIZES] + [list(C.CASES.values())]
    firsts = [C._data(0 if k % 3 == 0 else 40 * k) for k in range(len(trees))] if first else None
    lists = [C.host_results(t) for t in trees]
    dev, host, n = _paths(monkeypatch, ctx, lambda: H.results_hashes(ctx, lists, firsts))
    assert n == 1 and dev == host == _want(trees, firsts)


def test_host_layer_keeps_a_long_result_on_the_host(ctx, monkeypatch):
    """The tree holding a 16 KiB result stays on the host inside a device call; with a cap below every
    tree's longest result nothing is launched."""
    trees = [C.tree(20, 1), [C.CASES["data16384"]] + C.tree(5, 2), C.tree(64, 3)]
    assert max(len(r[1]) for t in (trees[0], trees[2]) for r in t) < 1000
    lists = [C.host_results(t) for t in trees]
    monkeypatch.setenv("TMV_DEVICE_RESULTS_MAX_DATA", "1000")
    dev, host, n = _paths(monkeypatch, ctx, lambda: H.results_hashes(ctx, lists))
    assert n == 1 and dev == host == _want(trees)
    monkeypatch.setenv("TMV_DEVICE_RESULTS_MAX_DATA", "0")
    only_long = [[C.CASES["data1"]], [C.CASES["data127"]]]
    dev, host, n = _paths(monkeypatch, ctx, lambda: H.results_hashes(ctx, [C.host_results(t) for t in only_long]))
    assert n == 0 and dev == host == _want(only_long)


def test_default_threshold_keeps_a_small_call_on_the_host(ctx, monkeypatch):
    monkeypatch.delenv("TMV_DEVICE_RESULTS_MIN", raising=False)
    trees = [C.tree(5, 5)]
    with _launch_counts(ctx) as launches:
        assert H.results_hashes(ctx, [C.host_results(t) for t in trees]) == _want(trees)
        assert launches() == 0


def test_verify_calls_on_both_paths(ctx, monkeypatch):
    items = C.block_results_items()
    dev, host, n = _paths(monkeypatch, ctx, lambda: H.block_results_verify(ctx, [it for it, _ in items]))
    assert n == 1 and dev == host == [w for _, w in items]
    params = C.consensus_params_items()
    dev, host, n = _paths(monkeypatch, ctx, lambda: H.consensus_params_verify(ctx, [it for it, _ in params]))
    assert n == 0 and dev == host == [w for _, w in params]


@pytest.mark.parametrize("window,depth", [(5, 2), (100, 1)])
def test_blocksync_replay_stateful_on_the_engine(ctx, monkeypatch, window, depth):
    """The honest chain and three wrong blocks, signatures verified by the engine, the result roots hashed on
    the device (the knob at 1: a 12-block chain is far below the default)."""
    scenarios = C.replay_scenarios()
    names = ("clean", "app_hash", "result_tampered", "proposer_before_time")
    monkeypatch.setenv("TMV_DEVICE_RESULTS_MIN", "1")
    with _launch_counts(ctx) as launches:
        C.check_replay(lambda st, bl, rec: chains.blocksync_replay_stateful(ctx, st, bl, rec, window=window,
                                                                            depth=depth, part_size=128),
                       scenarios, names)
        assert launches() >= len(names)


def test_kernel_timing_reports_the_launch(ctx):
    trees = [C.tree(100, 4)]
    with _launch_counts(ctx) as launches:
        _roots(ctx, trees)
        ms, n = ctx.kernel_timing_read("k_result_leaves")
        assert n == 1 and ms > 0
        assert launches() == 0
