"""Light blocks validated from their protobuf bytes, on the device:
tmv_merkle_wire_roots (k_span_leaves + k_valset_span_leaves + k_merkle_tree),
the device path of tmv_light_blocks_validate_wire, chains.statesync_backfill
and chains.verify_sequential_wire, against oracle/merkle_ref.py, the column
kernel (tmv_validator_set_hashes), the host path and the restatement
(tests/light_wire_ref.py).  The CPU twin is tests/test_light_wire_host.py."""
import contextlib
import ctypes
import dataclasses
import hashlib
import os
import random
import re

import numpy as np
import pytest

import light_wire_cases as W
import light_wire_ref as R
import merkle_ref as M
from tendermint_amd import chains, host as H
from tendermint_amd._native import NativeError, TMV_SPAN_PREHASH, TMV_SPAN_TAG
from tendermint_amd.testing.light_wire import encode_light_block

pytestmark = pytest.mark.gpu

TIMED = ("k_span_leaves", "k_valset_span_leaves", "k_merkle_leaves", "k_merkle_leaves_long", "k_merkle_tree_levels")
PERIOD, DRIFT = 3 * 3600 * 10**9, 10 * 10**9


@contextlib.contextmanager
def _launch_counts(ctx):
    """Kernel timing on inside the block (the launch counts tell which path a
    call took); nothing recorded is left behind for later tests."""
    ctx.kernel_timing(True)
    try:
        for k in TIMED:
            ctx.kernel_timing_read(k)
        yield lambda k: ctx.kernel_timing_read(k)[1]
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


def _span_item(data: bytes, pos: int, n: int, flags: int) -> bytes:
    span = data[pos:pos + n]
    if flags & TMV_SPAN_PREHASH:
        return hashlib.sha256(span).digest()
    return (bytes([flags & 0xFF]) if flags & TMV_SPAN_TAG else b"") + span


def _val_item(data: bytes, pos: int, n: int, power_at: int) -> bytes:
    """The substituted bytes of one validator leaf: 0a for byte 0, 10 for byte power_at."""
    span = bytearray(data[pos:pos + n])
    span[0] = 0x0A
    if power_at < n:
        span[power_at] = 0x10
    return bytes(span)


def _want(data, spans, vals, tree_off):
    items = [_span_item(data, *s) for s in spans] + [_val_item(data, *v) for v in vals]
    return [M.hash_from_byte_slices(items[tree_off[t]:tree_off[t + 1]]) for t in range(len(tree_off) - 1)]


KINDS = (0, TMV_SPAN_TAG | 0x0A, TMV_SPAN_TAG | 0x08, TMV_SPAN_PREHASH)


def test_wire_roots_every_length_alignment_and_tree_size(ctx):
    """One call over 1021 random bytes (no multiple of 4).  Validator leaves of
    every payload length (34, 35) x every power length (absent, 1 .. 10 bytes)
    x every byte alignment: messages of 37 .. 49 bytes; the shortest and the
    longest span the engine takes (2, 54); one at position 0 and one ending at
    the data's last byte.  Span leaves of all four kinds mixed in.  Trees of
    0 .. 129 leaves (both tree kernels) with a trailing empty tree; the leaf
    order puts the boundary between the two kinds inside a tree.  One launch of
    each leaf kernel."""
    rng = random.Random(23)
    data = bytes(rng.randrange(256) for _ in range(1021))
    vals = []
    for payload in (34, 35):
        for plen in range(0, 11):
            for a in range(4):
                n = 2 + payload + (1 + plen if plen else 0)
                pos = 4 * rng.randrange((len(data) - n - 3) // 4) + a
                vals.append((pos, n, 2 + payload))
    assert {1 + n for _, n, _ in vals} == set(range(37, 50))
    vals += [(0, 38, 36), (0, 36, 36), (len(data) - 48, 48, 37), (len(data) - 37, 37, 37), (len(data) - 2, 2, 2),
             (5, 54, 54), (6, 54, 2), (7, 3, 2), (len(data) - 54, 54, 53)]
    assert {p % 4 for p, _, _ in vals} == {0, 1, 2, 3}
    spans = []
    for n in (0, 1, 55, 56, 64, 119, 129):
        for flags in KINDS:
            spans.append((rng.randrange(len(data) - n), n, flags))
    spans += [(0, 64, 0), (len(data) - 57, 57, TMV_SPAN_PREHASH), (len(data), 0, 0)]
    sizes = [0, 1, 2, 3, 64, 65, 128, 129, 0]
    total = sum(sizes)
    n_spans = 1 + 2 + 3 + 64 + 30  # the boundary between the two kinds lies inside the tree of 65
    n_vals = total - n_spans
    assert n_spans >= len(spans) and n_vals >= len(vals)
    rng.shuffle(spans)
    rng.shuffle(vals)
    span_table = [spans[i % len(spans)] for i in range(n_spans)]
    val_table = [vals[i % len(vals)] for i in range(n_vals)]
    tree_off = np.zeros(len(sizes) + 1, np.uint32)
    tree_off[1:] = np.cumsum(sizes)
    with _launch_counts(ctx) as launches:
        got = [bytes(r) for r in ctx.merkle_wire_roots(data, np.array(span_table, np.uint32),
                                                       np.array(val_table, np.uint32), tree_off)]
        assert launches("k_span_leaves") == 1 and launches("k_valset_span_leaves") == 1
    assert got == _want(data, span_table, val_table, tree_off)
    assert got[0] == got[-1] == M.empty_hash()
    # either table empty
    off = np.array([0, 1, len(vals)], np.uint32)
    with _launch_counts(ctx) as launches:
        got = [bytes(r) for r in ctx.merkle_wire_roots(data, None, np.array(vals, np.uint32), off)]
        assert launches("k_span_leaves") == 0 and launches("k_valset_span_leaves") == 1
    assert got == _want(data, [], vals, off)
    off = np.array([0, 3, len(spans), len(spans)], np.uint32)
    with _launch_counts(ctx) as launches:
        got = [bytes(r) for r in ctx.merkle_wire_roots(data, np.array(spans, np.uint32), None, off)]
        assert launches("k_span_leaves") == 1 and launches("k_valset_span_leaves") == 0
    assert got == _want(data, spans, [], off) == [bytes(r) for r in ctx.merkle_span_roots(
        data, np.array(spans, np.uint32), off)]
    assert len(ctx.merkle_wire_roots(data, None, None, np.zeros(1, np.uint32))) == 0  # n_trees == 0


def _set(n, kinds, seed):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        key = bytes(rng.randrange(256) for _ in range(33 if kind == 3 else 32))
        power = rng.choice([0, 1, 127, 128, 300, 1 << 20, (1 << 55) // (n + 1), -1, -(1 << 40)])
        out.append(H.Validator(bytes(rng.randrange(256) for _ in range(20)), key, power, kind, rng.randrange(-5, 5)))
    return H.ValidatorSet(out, 0)


def _set_spans(sets):
    """The validator sets as one buffer of ValidatorSet messages and the spans of their validators."""
    data, table, tree_off = b"\x7f", [], [0]  # one byte in front: the first message starts unaligned
    for vs in sets:
        lb = H.LightBlock(None, vs)
        raw, fs = encode_light_block(lb)
        for i, v in enumerate(vs.validators):
            pk = next(f for f in fs if f.path == "validator_set.validators[%d].pub_key" % i)
            end = next((f.end for f in fs if f.path == "validator_set.validators[%d].voting_power" % i), pk.end)
            table.append((len(data) + pk.tag, end - pk.tag, pk.end - pk.tag))
        tree_off.append(len(table))
        data += raw
    return data, np.array(table, np.uint32).reshape(-1, 3), np.array(tree_off, np.uint32)


def test_wire_roots_equal_the_column_kernel(ctx):
    """ed25519 / sr25519 sets of 1, 2, 3, 65 and 150 validators: the roots from
    wire spans are tmv_validator_set_hashes' from columns."""
    sets = [_set(n, kinds, 100 + n) for n in (1, 2, 3, 65, 150) for kinds in ((0,), (1,), (0, 1))]
    sets = [H.ValidatorSet([dataclasses.replace(v, voting_power=abs(v.voting_power)) for v in s.validators], 0)
            for s in sets]
    data, table, tree_off = _set_spans(sets)
    got = [bytes(r) for r in ctx.merkle_wire_roots(data, None, table, tree_off)]
    assert got == chains.validator_set_hashes(ctx, sets) == [R.vals_hash(s.validators) for s in sets]


def test_wire_roots_of_secp256k1_and_mixed_sets_equal_the_light_path(ctx):
    """Sets holding secp256k1 keys are hashed on the host by the light path
    (ValidatorSetHashHost); light.VerifyAdjacent prints that hash when the
    header names another one.  The roots from wire spans are those hashes."""
    from tendermint_amd.testing.factory import make_light_chain
    trusted, (lb,) = make_light_chain(1, 4, W.CHAIN)
    sets = [_set(n, kinds, 200 + n) for n, kinds in ((1, (3,)), (4, (3,)), (7, (0, 3, 1)), (66, (3, 0)), (150, (1, 3)))]
    data, table, tree_off = _set_spans(sets)
    got = [bytes(r) for r in ctx.merkle_wire_roots(data, None, table, tree_off)]
    assert got == [R.vals_hash(s.validators) for s in sets]
    now = (lb.signed_header.header.time[0] + 5, 0)
    jobs = []
    for s in sets:
        other = W.resign(dataclasses.replace(lb, vals=s), validators_hash=b"\x13" * 32)
        jobs.append(H.LightJob(trusted.signed_header, None, other.signed_header, s, PERIOD, now, DRIFT,
                               mode=H.LIGHT_ADJACENT))
    for (kind, text), root in zip(H.light_verify_many(ctx, jobs), got):
        m = re.search(r"to match those that were supplied \(([0-9A-F]{64})\)", text)
        assert m and bytes.fromhex(m.group(1)) == root, text


def test_wire_roots_argument_errors(ctx):
    data = bytes(range(100))
    spans = np.array([(0, 10, 0), (1, 2, TMV_SPAN_TAG | 8)], np.uint32)
    vals = np.array([(0, 40, 36), (60, 40, 40), (3, 2, 2)], np.uint32)
    off = np.array([0, 3, 5], np.uint32)
    assert len(ctx.merkle_wire_roots(data, spans, vals, off)) == 2

    def bad(s=spans, v=vals, tree_off=off, d=data, **kw):
        with pytest.raises(NativeError, match=r"\(-1\)"):
            ctx.merkle_wire_roots(d, s, v, tree_off, **kw)

    def with_val(i, row):
        x = vals.copy()
        x[i] = row
        return x
    bad(v=with_val(0, (0, 55, 36)))                      # len > 54
    bad(v=with_val(0, (0, 1, 1)))                        # len < 2
    bad(v=with_val(0, (0, 0, 0)))
    bad(v=with_val(1, (60, 40, 1)))                      # power_at < 2
    bad(v=with_val(1, (60, 40, 0)))
    bad(v=with_val(1, (60, 40, 41)))                     # power_at > len
    bad(v=with_val(1, (61, 40, 40)))                     # pos + len > data_len
    bad(v=with_val(2, (100, 2, 2)))
    bad(v=with_val(2, (0xFFFFFFFF, 2, 2)))               # pos + len wraps in 32 bits
    bad(v=with_val(2, (0xFFFFFFE0, 40, 40)))
    bad(v=None, n_val_leaves=3)                          # null table
    bad(s=None, n_leaves=2)
    bad(d=None, data_len=100)                            # null data
    bad(n_leaves=(1 << 26) - 2, tree_off=np.array([0, 3, (1 << 26) + 1], np.uint32))  # n_leaves + n_val_leaves > 2^26
    bad(n_val_leaves=1 << 26, tree_off=np.array([0, 3, (1 << 26) + 2], np.uint32))
    bad(tree_off=np.array([0, 3, 4], np.uint32))         # does not end at n_leaves + n_val_leaves
    bad(tree_off=np.array([0, 3, 2], np.uint32))         # decreases
    bad(tree_off=np.array([1, 3, 5], np.uint32))         # does not start at 0
    bad(data_len=(1 << 30) + 1)                          # too many bytes
    # tmv_merkle_span_roots' own cases
    x = spans.copy()
    x[1] = (1, 2, 0x400)
    bad(s=x)                                             # an unknown flag bit
    x[1] = (1, 2, TMV_SPAN_TAG | TMV_SPAN_PREHASH | 8)
    bad(s=x)                                             # both flags
    x[1] = (1, 2, 8)
    bad(s=x)                                             # a tag byte without TAG
    x[1] = (99, 2, 0)
    bad(s=x)                                             # outside the data
    with pytest.raises(NativeError, match=r"\(-1\)"):    # the old entry point still refuses 0x400
        ctx.merkle_span_roots(data, np.array([(1, 2, 0x400)], np.uint32), np.array([0, 1], np.uint32))
    L = ctx._lib
    p = lambda a, t=ctypes.c_uint32: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    out = np.zeros(64, np.uint8)
    d = np.frombuffer(data, np.uint8)
    args = (p(d, ctypes.c_uint8), 100, p(spans), 2, p(vals), 3)
    assert L.tmv_merkle_wire_roots(ctx._h, *args, p(off), (1 << 26) + 1, p(out, ctypes.c_uint8)) == -1  # too many trees
    assert L.tmv_merkle_wire_roots(ctx._h, *args, None, 2, p(out, ctypes.c_uint8)) == -1
    assert L.tmv_merkle_wire_roots(ctx._h, *args, p(off), 2, None) == -1
    assert L.tmv_merkle_wire_roots(None, *args, p(off), 2, p(out, ctypes.c_uint8)) == -1
    assert [bytes(r) for r in ctx.merkle_wire_roots(data, spans, vals, off)] == \
        _want(data, [tuple(r) for r in spans.tolist()], [tuple(r) for r in vals.tolist()], off)  # the context still works


# ---- the host layer's device path ----
@pytest.fixture(scope="module")
def window():
    return W.window(40, 7)


def _struct_hashes(ctx, blocks):
    return H.header_hashes(ctx, [b.signed_header.header for b in blocks]), \
        chains.validator_set_hashes(ctx, [b.vals for b in blocks])


def test_device_path_equals_host_path_and_struct_path(ctx, window):
    """40 light blocks x 7 validators, the text-case mutations and not-handled
    blocks in the middle: one tmv_merkle_wire_roots call (one launch of each
    leaf kernel); verdicts, texts and hashes equal the host path's, the
    restatement's, and tmv_header_hashes / tmv_validator_set_hashes over the
    structs."""
    _, blocks, raws = window
    raws = list(raws)
    names = sorted(W.TEXT_CASES)
    for k, n in enumerate(names):
        raws[2 * k + 1] = W.encode(W.TEXT_CASES[n][0](blocks[2 * k + 1]))
    reasons = W.reason_cases(blocks[38])
    raws[38], raws[36] = reasons["key_unset"][0], raws[36][:-3]
    with _launch_counts(ctx) as launches:
        dev = H.light_blocks_validate_wire(ctx, W.CHAIN, raws, decode=True)
        assert launches("k_span_leaves") == 1 and launches("k_valset_span_leaves") == 1
        assert launches("k_merkle_leaves") == 0 and launches("k_merkle_leaves_long") == 0
    with _env(TMV_DEVICE_HASH_MIN=1000), _launch_counts(ctx) as launches:
        host = H.light_blocks_validate_wire(ctx, W.CHAIN, raws, decode=True)
        assert launches("k_span_leaves") == 0 and launches("k_valset_span_leaves") == 0
    strip = lambda vs: [(v.result, v.reason, v.error, v.hash, v.vals_hash) for v in vs]  # noqa: E731
    assert strip(dev) == strip(host)
    assert (dev[38].result, dev[38].reason, dev[36].reason) == (H.WIRE_NOT_HANDLED, "KEY", "TRUNCATED")
    for i, (v, raw) in enumerate(zip(dev, raws)):
        if v.result != H.WIRE_NOT_HANDLED:
            assert W.verdict(v) == W.expected(raw), i
    assert sum(v.result == H.WIRE_OK for v in dev) == 40 - len(names) - 2
    for k, n in enumerate(names):
        assert W.TEXT_CASES[n][1] in dev[2 * k + 1].error, n
    ok = [i for i, v in enumerate(dev) if v.result == H.WIRE_OK]
    hh, vh = _struct_hashes(ctx, [blocks[i] for i in ok])
    assert [dev[i].hash for i in ok] == hh and [dev[i].vals_hash for i in ok] == vh
    # below the threshold nothing is launched
    with _launch_counts(ctx) as launches:
        few = H.light_blocks_validate_wire(ctx, W.CHAIN, raws[:31])
        assert launches("k_valset_span_leaves") == 0
    assert strip(few) == strip(dev)[:31]


def test_go_made_light_blocks_on_the_device(ctx):
    """The Go-made light blocks of mbt_light.json: ValidatorsHash and header
    hash out of the device path (a threshold of 1 puts the small file there)."""
    lbs, _ = W.go_made_light_blocks()  # all 29 that have validators
    raws = [encode_light_block(lb)[0] for lb in lbs]
    with _env(TMV_DEVICE_HASH_MIN=1), _launch_counts(ctx) as launches:
        got = H.light_blocks_validate_wire(ctx, lbs[0].signed_header.header.chain_id, raws)
        assert launches("k_valset_span_leaves") == 1
    for lb, v in zip(lbs, got):
        assert (v.result, v.error) == (H.WIRE_OK, None)
        assert v.vals_hash == lb.signed_header.header.validators_hash
        assert v.hash == lb.signed_header.commit.block_id.hash


def _flat(r):
    n, err = r
    return n, None if err is None else (err.from_height, err.to_height, err.kind, err.reason)


def test_drivers_on_the_device(ctx, window):
    """verify_sequential_wire equals verify_sequential on a signed chain of 40
    headers x 7 validators, clean and with one bad signature: the view
    pointers feed tmv_light_verify_many directly.  statesync_backfill over the
    same chain, clean and failing."""
    trusted, blocks, raws = window
    now = (blocks[-1].signed_header.header.time[0] + 5, 0)
    want = _flat(chains.verify_sequential(ctx, trusted, blocks, PERIOD, now, DRIFT, window=40))
    assert want == (40, None)
    with _launch_counts(ctx) as launches:
        assert _flat(chains.verify_sequential_wire(ctx, trusted, raws, PERIOD, now, DRIFT, window=40)) == want
        assert launches("k_valset_span_leaves") == 1
    assert _flat(chains.verify_sequential_wire(ctx, trusted, raws, PERIOD, now, DRIFT, window=16)) == want
    sigs = list(blocks[33].signed_header.commit.signatures)
    s = bytearray(sigs[4].signature)
    s[9] ^= 4
    sigs[4] = dataclasses.replace(sigs[4], signature=bytes(s))
    bad = list(blocks)
    bad[33] = dataclasses.replace(blocks[33], signed_header=H.SignedHeader(
        blocks[33].signed_header.header, dataclasses.replace(blocks[33].signed_header.commit, signatures=sigs)))
    want = _flat(chains.verify_sequential(ctx, trusted, bad, PERIOD, now, DRIFT, window=40))
    assert want[0] == 33 and want[1] is not None
    assert _flat(chains.verify_sequential_wire(ctx, trusted, [W.encode(b) for b in bad], PERIOD, now, DRIFT,
                                               window=40)) == want
    top = blocks[-1].signed_header.commit.block_id.hash
    heights = [b.height for b in blocks[::-1]]
    with _launch_counts(ctx) as launches:
        assert chains.statesync_backfill(ctx, W.CHAIN, raws[::-1], top, window=40) == (40, None, heights[1:])
        assert launches("k_valset_span_leaves") == 1
    newest = raws[::-1]
    newest[20] = W.encode(W.resign(blocks[::-1][20], app_hash=b"\x03" * 20))
    n, err, _ = chains.statesync_backfill(ctx, W.CHAIN, newest, top, window=40)
    assert n == 20 and err[0] == heights[20] and err[1].startswith("received invalid light block. Expected hash ")
    newest[7] = W.encode(W.TEXT_CASES["address_size_4"][0](blocks[::-1][7]))
    n, err, _ = chains.statesync_backfill(ctx, W.CHAIN, newest, top, window=40)
    assert (n, err[0]) == (7, heights[7]) and err[1].startswith(
        "received invalid light block: invalid validator set: invalid validator #4: ")
