"""Blocks validated from their protobuf bytes, on the device:
tmv_merkle_span_roots (k_span_leaves + k_merkle_tree), the device path of
tmv_blocks_validate_wire and chains.blocksync_replay_wire against the
restatement of the reference (tests/merkle_ref.py, tests/commit_hash_ref.py).
The CPU twin is tests/test_block_wire_host.py."""
import contextlib
import ctypes
import dataclasses
import hashlib
import os
import random

import numpy as np
import pytest

import block_wire_cases as W
import blocks_cases as C
import commit_hash_ref as R
import merkle_ref as M
from tendermint_amd import chains, host as H
from tendermint_amd import _native
from tendermint_amd._native import NativeError, TMV_SPAN_PREHASH, TMV_SPAN_TAG
from tendermint_amd.testing.block_wire import encode_block
from tendermint_amd.testing.blocks import make_full_chain

pytestmark = pytest.mark.gpu

TIMED = ("k_span_leaves", "k_commit_leaves", "k_merkle_leaves_long", "k_merkle_leaves", "k_merkle_tree_levels")


@contextlib.contextmanager
def _launch_counts(ctx):
    """Kernel timing on inside the block (the launch counts tell which path a
    call took); nothing recorded is left behind for later tests."""
    ctx.kernel_timing(True)
    try:
        for k in TIMED:
            ctx.kernel_timing_read(k)
        yield lambda k="k_span_leaves": ctx.kernel_timing_read(k)[1]
    finally:
        ctx.kernel_timing(False)
        for k in TIMED:
            ctx.kernel_timing_read(k)


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _leaf_item(data: bytes, pos: int, n: int, flags: int) -> bytes:
    """What merkle.HashFromByteSlices is given for one span."""
    span = data[pos:pos + n]
    if flags & TMV_SPAN_PREHASH:
        return hashlib.sha256(span).digest()
    return (bytes([flags & 0xFF]) if flags & TMV_SPAN_TAG else b"") + span


def _want(data, spans, tree_off):
    return [M.hash_from_byte_slices([_leaf_item(data, *spans[i]) for i in range(tree_off[t], tree_off[t + 1])])
            for t in range(len(tree_off) - 1)]


LENGTHS = [0, 1] + list(range(53, 58)) + list(range(62, 67)) + list(range(117, 122)) + [127, 128, 129]
KINDS = (0, TMV_SPAN_TAG | 0x0A, TMV_SPAN_TAG | 0x08, TMV_SPAN_PREHASH)


def test_span_roots_every_boundary_alignment_kind_and_tree_size(ctx):
    """The SHA-256 block boundaries with the one-byte prefix (55/56, 63/64/65,
    119/120, 127/128), with prefix plus tag (54/55, 62/63, 118/119) and of the
    inner hash (55/56, 64, 119/120, 128); each length plain, tagged and
    pre-hashed at every byte alignment; a span at position 0 and spans ending
    at the data's last byte, whose length is no multiple of 4; trees of
    0 .. 129 leaves (both tree kernels).  One call, one leaf launch."""
    rng = random.Random(4)
    data = bytes(rng.randrange(256) for _ in range(1021))
    spans = []
    for n in LENGTHS:
        for flags in KINDS:
            for a in range(4):
                pos = 4 * rng.randrange((len(data) - n - 3) // 4) + a
                spans.append((pos, n, flags))
    for flags in KINDS:
        spans += [(0, 64, flags), (0, 0, flags), (len(data), 0, flags)]
        spans += [(len(data) - n, n, flags) for n in (1, 57, 66, 129)]
    spans.append((0, len(data), 0))             # the whole buffer, overlapping everything
    spans.append((0, len(data), TMV_SPAN_PREHASH))
    assert {p % 4 for p, n, _ in spans if n} == {0, 1, 2, 3} and any(p + n == len(data) and n for p, n, _ in spans)
    sizes = [0, 1, 2, 3, 64, 65, 128, 129, 0]
    total = sum(sizes)
    assert total >= len(spans)
    rng.shuffle(spans)
    table = [spans[i % len(spans)] for i in range(total)]  # every span at least once
    tree_off = np.zeros(len(sizes) + 1, np.uint32)
    tree_off[1:] = np.cumsum(sizes)
    with _launch_counts(ctx) as launches:
        got = [bytes(r) for r in ctx.merkle_span_roots(data, np.array(table, np.uint32), tree_off)]
        assert launches() == 1
    assert got == _want(data, table, tree_off)
    assert got[0] == got[-1] == M.empty_hash()


def test_span_roots_long_spans_and_trees_only_of_empty_leaves(ctx):
    rng = random.Random(5)
    data = bytes(rng.randrange(256) for _ in range(70001))
    table = [(1, 70000, 0), (3, 4097, TMV_SPAN_PREHASH), (2, 65536, TMV_SPAN_TAG | 0xFF), (0, 0, 0), (7, 0, 0)]
    tree_off = np.array([0, 3, 5, 5], np.uint32)
    assert [bytes(r) for r in ctx.merkle_span_roots(data, np.array(table, np.uint32), tree_off)] == \
        _want(data, table, tree_off)
    # no data at all: empty leaves and empty trees
    table = [(0, 0, 0), (0, 0, TMV_SPAN_PREHASH), (0, 0, TMV_SPAN_TAG | 0x0A)]
    tree_off = np.array([0, 0, 3], np.uint32)
    assert [bytes(r) for r in ctx.merkle_span_roots(None, np.array(table, np.uint32), tree_off, data_len=0)] == \
        _want(b"", table, tree_off)
    assert len(ctx.merkle_span_roots(data, None, np.zeros(1, np.uint32))) == 0  # n_trees == 0


def test_span_roots_equal_the_column_kernel(ctx):
    """ENCODER_CASES of blocks_cases as encoded CommitSigs, given as spans:
    the roots tmv_commit_hashes computes from the same entries as columns."""
    cases = list(C.ENCODER_CASES.values())
    commits = [cases] + [[c] for c in cases] + [[], cases[:7]]
    data, table, tree_off = b"\xee", [], [0]  # one byte in front: the spans start unaligned
    for c in commits:
        for s in c:
            enc = R.commit_sig_bytes(*s)
            table.append((len(data), len(enc), 0))
            data += enc
        tree_off.append(len(table))
    got = [bytes(r) for r in ctx.merkle_span_roots(data, np.array(table, np.uint32), np.array(tree_off, np.uint32))]
    assert got == [bytes(r) for r in ctx.commit_hashes(*C.columns(commits))] == [R.commit_hash_of_sigs(c) for c in commits]


def test_span_roots_argument_errors(ctx):
    data = bytes(range(100))
    good = np.array([(0, 10, 0), (5, 95, TMV_SPAN_PREHASH), (1, 2, TMV_SPAN_TAG | 8)], np.uint32)
    off = np.array([0, 2, 3], np.uint32)
    assert len(ctx.merkle_span_roots(data, good, off)) == 2

    def bad(spans=good, tree_off=off, d=data, **kw):
        with pytest.raises(NativeError, match=r"\(-1\)"):
            ctx.merkle_span_roots(d, spans, tree_off, **kw)

    def with_span(i, row):
        s = good.copy()
        s[i] = row
        return s
    bad(d=None, data_len=100)                                 # null data
    bad(spans=None, n_leaves=3)                               # null spans
    bad(spans=with_span(1, (5, 96, 0)))                       # pos + len > data_len
    bad(spans=with_span(0, (101, 0, 0)))
    bad(spans=with_span(0, (0xFFFFFFFF, 2, 0)))               # pos + len wraps in 32 bits
    bad(spans=with_span(2, (1, 2, TMV_SPAN_TAG | TMV_SPAN_PREHASH | 8)))  # both flags
    bad(spans=with_span(2, (1, 2, 0x400)))                    # an unknown flag bit
    bad(spans=with_span(2, (1, 2, 8)))                        # a tag byte without TAG
    bad(tree_off=np.array([1, 2, 3], np.uint32))              # does not start at 0
    bad(tree_off=np.array([0, 3, 2], np.uint32))              # decreases
    bad(tree_off=np.array([0, 2, 2], np.uint32))              # does not end at n_leaves
    bad(tree_off=np.array([0, 2, 4], np.uint32))
    bad(n_leaves=(1 << 26) + 1)                               # too many leaves
    bad(data_len=(1 << 30) + 1)                               # too many bytes
    L, u32p = ctx._lib, ctypes.POINTER(ctypes.c_uint32)
    out = np.zeros(64, np.uint8)
    p = lambda a, t=ctypes.c_uint8: a.ctypes.data_as(ctypes.POINTER(t))
    d = np.frombuffer(data, np.uint8)
    assert L.tmv_merkle_span_roots(ctx._h, p(d), 100, p(good, ctypes.c_uint32), 3, p(off, ctypes.c_uint32),
                                   (1 << 26) + 1, p(out)) == -1  # too many trees
    assert L.tmv_merkle_span_roots(ctx._h, p(d), 100, p(good, ctypes.c_uint32), 3, None, 2, p(out)) == -1
    assert L.tmv_merkle_span_roots(ctx._h, p(d), 100, p(good, ctypes.c_uint32), 3, p(off, ctypes.c_uint32), 2,
                                   None) == -1
    assert L.tmv_merkle_span_roots(None, p(d), 100, p(good, ctypes.c_uint32), 3, p(off, ctypes.c_uint32), 2,
                                   p(out)) == -1
    assert len(ctx.merkle_span_roots(data, good, off)) == 2  # and the context still works


# ---- the host layer's device path ----
@pytest.fixture(scope="module")
def window():
    """40 unsigned blocks with their real encoding (ValidateBasic reads no signature)."""
    _, blocks, _ = make_full_chain(40, 7, C.CHAIN, seed=8, txs=(0, 5), tx_len=(0, 300), absent=(3,), sign=False,
                                   wire=True)
    return blocks


def test_device_path_equals_the_struct_path(ctx, window):
    raws = [b.raw for b in window]
    want = [W.expected(b) for b in window]
    assert all(e is None for e, _ in want)
    with _launch_counts(ctx) as launches:
        got = H.blocks_validate_wire(ctx, raws, 65536, decode=True)
        assert launches() == 1 and launches("k_commit_leaves") == 0  # one leaf launch for the whole window
        assert [W.verdict_pair(v) for v in got] == want == H.blocks_validate_basic(ctx, window)
        assert launches() == 0 and launches("k_commit_leaves") == 1  # the struct path's own kernels
        assert [v.block for v in got] == window
        assert [v.part_set_header for v in got] == [R.part_set_header(r, 65536) for r in raws]
        assert [W.verdict_pair(v) for v in H.blocks_validate_wire(ctx, raws[:31])] == want[:31]
        assert launches() == 0  # below TMV_DEVICE_BLOCK_MIN: the host path
        with _env(TMV_DEVICE_BLOCK_MIN=1000):
            assert [W.verdict_pair(v) for v in H.blocks_validate_wire(ctx, raws)] == want
            assert launches() == 0
        with _env(TMV_DEVICE_BLOCK_MIN=2):
            assert [W.verdict_pair(v) for v in H.blocks_validate_wire(ctx, raws[:3])] == want[:3]
            assert launches() == 1


def test_device_path_validate_basic_mutations(ctx, window):
    """Every ValidateBasic mutation in the middle of the window, on the device
    and with the threshold raised: the struct path's texts and hashes."""
    rng = random.Random(79)
    mutated, names = list(window), {}
    for name, (fn, text) in C.MUTATIONS.items():
        if name == "evidence_tampered":  # takes the block out of the wire path: the next test
            continue
        while True:
            i = rng.randrange(5, 35)
            sigs = window[i].last_commit.signatures
            if i not in names and window[i].txs and all(sigs[j].block_id_flag == H.BLOCK_ID_FLAG_COMMIT
                                                        for j in (0, 1, -1)):
                break
        mutated[i], names[i] = fn(window[i]), (name, text)
    raws = [encode_block(b)[0] for b in mutated]
    want = [W.expected(b) for b in mutated]
    for i, (name, text) in names.items():
        assert text in want[i][0], name
    with _launch_counts(ctx) as launches:
        got = H.blocks_validate_wire(ctx, raws)
        assert launches() == 1
        assert [W.verdict_pair(v) for v in got] == want == H.blocks_validate_basic(ctx, mutated)
        assert [v.result for v in got] == [H.WIRE_INVALID if i in names else H.WIRE_OK for i in range(40)]
        launches()
        with _env(TMV_DEVICE_BLOCK_MIN=1000):
            assert [W.verdict_pair(v) for v in H.blocks_validate_wire(ctx, raws)] == want
        assert launches() == 0


def test_device_path_blocks_not_handled_and_long_transactions(ctx, window):
    raws = [b.raw for b in window]
    want = [W.expected(b) for b in window]
    raws[9] = encode_block(dataclasses.replace(window[9], evidence=[b"\x0a\x02ev"]))[0]
    raws[20] = W.rule_mutations(window[20])["padded_varint"][0]
    long_tx = dataclasses.replace(window[30], txs=[b"t" * 5000, b"u"])
    long_tx = dataclasses.replace(long_tx, header=dataclasses.replace(long_tx.header, data_hash=R.txs_hash(long_tx.txs)))
    raws[30], want[30] = encode_block(long_tx)[0], W.expected(long_tx)
    assert want[30][0] is None
    with _launch_counts(ctx) as launches:
        for knob in (16, 1024, 1 << 20):  # the long block's transactions on the host, then on the device
            with _env(TMV_DEVICE_WIRE_MAX_TX=knob):
                got = H.blocks_validate_wire(ctx, raws)
            assert launches() == 1
            assert [(got[i].result, got[i].reason, got[i].error, got[i].hash) for i in (9, 20)] == \
                [(H.WIRE_NOT_HANDLED, "EVIDENCE", None, None), (H.WIRE_NOT_HANDLED, "VARINT", None, None)]
            assert [W.verdict_pair(v) for i, v in enumerate(got) if i not in (9, 20)] == \
                [w for i, w in enumerate(want) if i not in (9, 20)], knob


# ---- the driver and the views ----
@pytest.fixture(scope="module")
def chain():
    vals, blocks, ids = make_full_chain(40, 5, C.CHAIN, seed=43, txs=(0, 5), wire=True)
    return vals, blocks, ids


def test_blocksync_replay_wire_clean_and_failing(ctx, chain):
    vals, blocks, ids = chain
    raws = [b.raw for b in blocks]
    for window in (16, 600):
        assert chains.blocksync_replay_wire(ctx, C.CHAIN, vals, raws, H.BlockID(), window=window) == (39, None) == \
            chains.blocksync_replay_full(ctx, C.CHAIN, vals, blocks, H.BlockID(), window=window)
    # a block that is wrong and properly signed
    edit = {23: lambda h: dataclasses.replace(h, data_hash=C._flip(h.data_hash))}
    vals, bad, _ = make_full_chain(40, 5, C.CHAIN, seed=43, txs=(0, 5), wire=True, header_edit=edit)
    want = C.oracle_replay(C.SigCache(), vals, bad[:26], H.BlockID())
    assert want[0] == 22 and want[1][0] == 23 and want[1][1].startswith("wrong Header.DataHash. Expected ")
    assert chains.blocksync_replay_wire(ctx, C.CHAIN, vals, [b.raw for b in bad], H.BlockID(), window=16) == want == \
        chains.blocksync_replay_full(ctx, C.CHAIN, vals, bad, H.BlockID(), window=16)


def test_view_commits_verify_by_pointer(ctx, chain):
    """tmv_block_views_block(v, i)->last_commit put straight into a
    tmv_commit_job: the commits of the views verify as the originals do."""
    vals, blocks, ids = chain
    L = H._setup_block_wire(H._setup_many(H._setup(_native.lib())))
    w = H.WireWindow([b.raw for b in blocks])
    views = ctypes.c_void_p()
    assert L.tmv_blocks_parse_wire(ctypes.cast(w.data, H._u8p), w.off, w.n, None, ctypes.byref(views)) == 0
    try:
        # block h + 1 carries the commit for block h; the last one is tampered in the bytes' copy below
        jobs = [H.CommitJob(H.MODE_LIGHT, C.CHAIN, vals, ids[i], blocks[i].height, None) for i in range(39)]
        pj = H.PreparedJobs(jobs)
        for i in range(39):
            pj.arr[i].commit = L.tmv_block_views_block(views, i + 1).contents.last_commit
        H.run_prepared_jobs(ctx, pj)
        assert pj.decode() == [None] * 39
        pj = H.PreparedJobs(jobs[:2])
        pj.arr[0].commit = L.tmv_block_views_block(views, 3).contents.last_commit  # another block's commit
        pj.arr[1].commit = L.tmv_block_views_block(views, 2).contents.last_commit
        H.run_prepared_jobs(ctx, pj)
        got = pj.decode()
        assert got[0] is not None and "wrong" in got[0] and got[1] is None
    finally:
        L.tmv_block_views_free(views)
