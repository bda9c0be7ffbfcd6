"""tmv_merkle_value_ops on the device (k_merkle_digests_long and
k_merkle_value_ops) and the device path of tmv_proof_ops_verify /
tmv_tx_proofs_validate, bit for bit against the restatement of the reference
(tests/proof_ops_ref.py).  The reference items are built once per module."""
import hashlib
import os
import random

import numpy as np
import pytest

import merkle_proof_ref as P
import proof_ops_cases as C
import proof_ops_ref as R
from tendermint_amd import _native
from tendermint_amd import host as H
from tendermint_amd._native import NativeError
from tendermint_amd.testing import simple_map as SM

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "proof_ops_vectors.json")

# 21: the message reaches 56 bytes (a second padding block); 30: 64 bytes; 84/85, 92/93: the same edges one block
# later; 128: a two-byte uvarint
KEY_LENS = (0, 1, 20, 21, 28, 29, 30, 84, 85, 92, 93, 127, 128, 300)
VALUE_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 511, 512, 513, 70001)
TREES = (1, 2, 3, 5, 100)
OUTPUTS = ("value_digest", "kv_hash_calc", "leaf_ok", "root_calc", "root_nil", "status", "fail_op")


def _bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


class Item:
    """One engine item: value, [proof_ops_ref.ValueOp], the expected root."""

    def __init__(self, value, ops, root):
        self.value, self.ops, self.root = value, ops, root

    def with_op(self, j, **kw):
        op = self.ops[j]
        d = dict(total=op.proof.total, index=op.proof.index, leaf_hash=op.proof.leaf_hash, aunts=list(op.proof.aunts))
        d.update(kw)
        ops = list(self.ops)
        ops[j] = R.ValueOp(op.key, P.Proof(d["total"], d["index"], d["leaf_hash"], d["aunts"]))
        return Item(self.value, ops, self.root)


def _timing_off(ctx):
    """Forget what these tests' launches recorded (other tests count their own launches), then stop recording."""
    for k in ("k_merkle_digests_long", "k_merkle_value_ops", "k_merkle_leaves_long", "k_merkle_verify_proofs"):
        ctx.kernel_timing_read(k)
    ctx.kernel_timing(False)


def _flip(b, at=0):
    return b[:at] + bytes([b[at] ^ 0x20]) + b[at + 1:]


def _make_items():
    rng = random.Random(31)
    vals = list(VALUE_LENS)
    rng.shuffle(vals)  # later values start unaligned
    items = []
    for i in range(64):  # one wave, items of 1, 2, 3 and 4 ops side by side
        n_ops = 1 + i % 4
        levels = []
        for j in range(n_ops):
            key = _bytes(rng, KEY_LENS[(i + 3 * j) % len(KEY_LENS)])
            pairs = {b"f%04d" % k: _bytes(rng, 6) for k in range(TREES[(i + j) % len(TREES)] - 1)}
            pairs[key] = _bytes(rng, vals[i % len(vals)]) if j == 0 else b""
            levels.append((pairs, key))
        it = SM.nested(levels, P.proofs_from_byte_slices)
        ops = [R.ValueOp(op.key, P.Proof(op.proof.total, op.proof.index, op.proof.leaf_hash, op.proof.aunts))
               for op in it.ops]
        items.append(Item(it.value, ops, it.root))
    assert {len(it.value) for it in items} == set(VALUE_LENS)
    assert {len(op.key) for it in items for op in it.ops} == set(KEY_LENS)
    assert {op.proof.total for it in items for op in it.ops} == set(TREES)
    return items


@pytest.fixture(scope="module")
def items():
    return _make_items()


def pack(items):
    value = b"".join(it.value for it in items)
    ops = [op for it in items for op in it.ops]
    aunts = b"".join(a for op in ops for a in op.proof.aunts)
    cum = lambda lens: np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.uint32)  # noqa: E731
    return dict(
        value=np.frombuffer(value, np.uint8), value_off=cum([len(it.value) for it in items]),
        op_off=cum([len(it.ops) for it in items]),
        key=np.frombuffer(b"".join(op.key for op in ops), np.uint8), key_off=cum([len(op.key) for op in ops]),
        total=np.array([op.proof.total for op in ops], np.int64), index=np.array([op.proof.index for op in ops], np.int64),
        leaf_hash=np.frombuffer(b"".join(op.proof.leaf_hash for op in ops), np.uint8),
        aunts=np.frombuffer(aunts, np.uint8), aunt_off=cum([len(op.proof.aunts) for op in ops]),
        root=np.frombuffer(b"".join(it.root for it in items), np.uint8))


def check(ctx, items, flags=0, skip=()):
    """One engine call against the restatement, output by output."""
    ok, out = ctx.merkle_value_ops(**pack(items), flags=flags, skip=skip)
    want = [R.engine_expect(it.value, it.ops, it.root) for it in items]
    per_op = [x for w in want for x in w[0]]
    exp = {
        "value_digest": b"".join(hashlib.sha256(it.value).digest() for it in items),
        "kv_hash_calc": b"".join(kv for kv, _, _ in per_op),
        "leaf_ok": bytes(1 if lo else 0 for _, lo, _ in per_op),
        "root_calc": b"".join(r if r is not None else bytes(32) for _, _, r in per_op),
        "root_nil": bytes(1 if r is None else 0 for _, _, r in per_op),
        "status": [w[1][0] for w in want],
        "fail_op": [w[1][1] for w in want],
    }
    for name in OUTPUTS:
        if name in skip:
            assert out[name] is None
        elif name in ("status", "fail_op"):
            assert out[name].tolist() == exp[name], name
        else:
            assert out[name].tobytes() == exp[name], name
    assert ok == all(s == 0 for s in exp["status"])
    return exp


def test_engine_all_shapes(ctx, items):
    ctx.kernel_timing(True)
    try:
        for k in ("k_merkle_digests_long", "k_merkle_value_ops"):
            ctx.kernel_timing_read(k)
        exp = check(ctx, items)
        assert exp["status"] == [0] * len(items)
        for k in ("k_merkle_digests_long", "k_merkle_value_ops"):
            assert ctx.kernel_timing_read(k)[1] == 1
    finally:
        _timing_off(ctx)


def test_engine_corruptions(ctx, items):
    four = next(it for it in items if len(it.ops) == 4 and len(it.ops[0].proof.aunts) >= 2)
    deep = next(it for it in items if len(it.ops) == 2 and len(it.ops[1].proof.aunts) >= 2)
    h32 = bytes(range(32))
    bad = [four.with_op(j, leaf_hash=_flip(four.ops[j].proof.leaf_hash, 5 * j)) for j in range(4)]
    bad += [four.with_op(0, leaf_hash=_flip(four.ops[0].proof.leaf_hash)).with_op(3, leaf_hash=h32)]  # the first one wins
    for it, j in ((four, 0), (deep, 1)):
        pr = it.ops[j].proof
        bad += [
            it.with_op(j, aunts=[_flip(pr.aunts[0], 31)] + pr.aunts[1:]),     # a flipped aunt
            it.with_op(j, aunts=pr.aunts[:-1] + [_flip(pr.aunts[-1])]),
            it.with_op(j, index=pr.total), it.with_op(j, index=pr.total + 5),  # index >= total
            it.with_op(j, total=0), it.with_op(j, total=0, index=0),
            it.with_op(j, total=-1), it.with_op(j, index=-1), it.with_op(j, total=-3, index=-3),
            it.with_op(j, aunts=pr.aunts + [h32]), it.with_op(j, aunts=pr.aunts[:-1]),  # one aunt too many / too few
            it.with_op(j, aunts=[]),
        ]
    bad += [Item(four.value, four.ops, _flip(four.root, 31)), Item(deep.value, deep.ops, h32),
            Item(four.value + b"x", four.ops, four.root), Item(b"", deep.ops, deep.root)]
    mixed = []
    for k, b in enumerate(bad):  # good items between the bad ones
        mixed += [b, items[k % len(items)]]
    exp = check(ctx, mixed)
    assert set(exp["status"]) == {0, 3, 4}
    assert exp["status"][0:8:2] == [3, 3, 3, 3] and exp["fail_op"][0:8:2] == [0, 1, 2, 3] and exp["fail_op"][8] == 0
    # a nil middle root is passed on as the empty string: the next op's kv hash is that of SHA-256("")
    nil_mid = four.with_op(0, index=four.ops[0].proof.total)
    _, out = ctx.merkle_value_ops(**pack([nil_mid]))
    assert out["root_nil"].tolist()[0] == 1 and out["kv_hash_calc"][1].tobytes() == four.ops[1].kv_hash(b"")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_engine_item_counts(ctx, items, n):
    many = [items[(7 * k) % len(items)] for k in range(n)]
    if n > 2:
        many[n // 2] = many[n // 2].with_op(0, leaf_hash=bytes(32))
        many[n - 1] = Item(many[n - 1].value, many[n - 1].ops, bytes(32))
    exp = check(ctx, many)
    assert n <= 2 or (exp["status"][n // 2], exp["status"][n - 1]) == (3, 4)


@pytest.mark.parametrize("skip", OUTPUTS)
def test_engine_null_outputs(ctx, items, skip):
    check(ctx, items[:33] + [items[0].with_op(0, leaf_hash=bytes(32))], skip=(skip,))
    check(ctx, items[:5], skip=tuple(o for o in OUTPUTS if o != skip))


@pytest.mark.parametrize("lpw", [0, 8, 16, 32, 64])
def test_value_digests_at_every_leaves_per_wave(ctx, items, lpw):
    many = [items[(5 * k + 1) % len(items)] for k in range(130)]  # more than one workgroup at every setting
    ok, out = ctx.merkle_value_ops(**pack(many), flags=_native.merkle_lpw(lpw), skip=OUTPUTS[1:])
    assert ok and out["value_digest"].tobytes() == b"".join(hashlib.sha256(it.value).digest() for it in many)


def test_argument_errors(ctx, items):
    base = pack(items[:6])

    def bad(**kw):
        a = dict(base)
        flags = kw.pop("flags", 0)
        a.update(kw)
        with pytest.raises(NativeError, match=r"\(-1\)"):
            ctx.merkle_value_ops(**a, flags=flags)

    for name in ("value", "key", "aunts", "leaf_hash", "root"):  # null pointers
        bad(**{name: None})
    for name in ("value_off", "op_off", "key_off", "aunt_off"):
        off = base[name].copy()
        off[0] = 1
        bad(**{name: off})            # does not start at 0
        off = base[name].copy()
        off[2], off[3] = max(off[2], off[3]) + 1, off[2]
        bad(**{name: off})            # decreases
    off = base["op_off"].copy()
    off[2] = off[1]
    bad(op_off=off)                   # an item without ops
    too = base["value_off"].copy()
    too[-1] = (1 << 30) + 1
    bad(value_off=too)                # more than 2^30 bytes of values
    too = base["key_off"].copy()
    too[-1] = (1 << 30) + 1
    bad(key_off=too)
    too = base["aunt_off"].copy()
    too[-1] = (1 << 28) + 1
    bad(aunt_off=too)                 # more than 2^28 aunts
    too = base["op_off"].copy()
    too[-1] = (1 << 26) + 1
    bad(op_off=too)                   # more than 2^26 ops: refused before key_off or aunt_off is read
    # more than 2^26 items: the count is refused before any offset is read, so the small arrays do
    import ctypes
    u8, u32, i64 = (lambda a, t=t: a.ctypes.data_as(ctypes.POINTER(t))
                    for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_int64))
    b = {k: np.ascontiguousarray(v) for k, v in base.items()}
    rc = _native.lib().tmv_merkle_value_ops(
        ctx.handle, 0, (1 << 26) + 1, u8(b["value"]), u32(b["value_off"]), u32(b["op_off"]), u8(b["key"]),
        u32(b["key_off"]), i64(b["total"]), i64(b["index"]), u8(b["leaf_hash"]), u8(b["aunts"]), u32(b["aunt_off"]),
        u8(b["root"]), None, None, None, None, None, None, None)
    assert rc == -1 and "tmv_merkle_value_ops" in _native.last_error()
    bad(flags=1)
    bad(flags=_native.merkle_lpw(24))
    ok, _ = ctx.merkle_value_ops(**base)  # and the context still works
    assert ok
    empty = {k: (np.zeros(1, np.uint32) if k.endswith("_off") else np.zeros(0, v.dtype)) for k, v in base.items()}
    assert ctx.merkle_value_ops(**empty)[0]  # an empty call


@pytest.mark.parametrize("knob", ["0", None], ids=["device", "default"])
def test_host_layer(ctx, monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("TMV_DEVICE_PROOF_OPS_MIN", raising=False)
    else:
        monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MIN", knob)
    ctx.kernel_timing(True)
    try:
        for k in ("k_merkle_value_ops", "k_merkle_verify_proofs"):
            ctx.kernel_timing_read(k)
        C.check_proof_ops(ctx, None)
        C.check_tx_proofs(ctx, None)
        ops, txs = C.load_golden(GOLDEN)
        assert H.proof_ops_verify(ctx, [it for _, it, _ in ops]) == [w for _, _, w in ops]
        assert H.tx_proofs_validate(ctx, [t for _, t, _ in txs]) == [w for _, _, w in txs]
        launches = [ctx.kernel_timing_read(k)[1] for k in ("k_merkle_value_ops", "k_merkle_verify_proofs")]
        if knob == "0":
            assert launches[0] >= 2 and launches[1] >= 2  # the calls did reach the engine
    finally:
        _timing_off(ctx)


def test_host_layer_equals_the_cpu_build(ctx, monkeypatch):
    import ctypes
    cpu = ctypes.CDLL(os.path.join(REPO, "oracle", "_build", "libproofopshost.so"))
    monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MIN", "0")
    its = [it for _, it, _ in C.proof_ops_cases()]
    txs = [t for _, t, _ in C.tx_cases()]
    assert H.proof_ops_verify(ctx, its) == H.proof_ops_verify(None, its, lib=cpu)
    assert H.tx_proofs_validate(ctx, txs) == H.tx_proofs_validate(None, txs, lib=cpu)


def test_host_layer_windows_at_the_default_threshold(ctx, monkeypatch):
    """A call above the default threshold goes to the device unasked, in more than one window of 16,384 ops;
    the items around the window's edge and the last one keep their own results."""
    monkeypatch.delenv("TMV_DEVICE_PROOF_OPS_MIN", raising=False)
    cases = C.proof_ops_cases()
    good, bad_leaf, bad_root = cases[1][1], cases[10][1], cases[11][1]   # 2 ops each
    assert C.expected(good) is None and "leaf hash mismatch" in C.expected(bad_leaf)
    n = 8200                                                            # 16,400 ops: two windows
    items = [good] * n
    marks = {0: bad_leaf, 8190: bad_root, 8191: bad_leaf, 8192: bad_root, 8193: bad_leaf, n - 1: bad_root}
    for k, it in marks.items():
        items[k] = it
    txs = [t for _, t, _ in C.tx_cases()]
    tx_want = [w for _, _, w in C.tx_cases()]
    reps = 900             # about 20 of the cases reach a hash in the engine's layout: more than one window of them
    ctx.kernel_timing(True)
    try:
        for k in ("k_merkle_value_ops", "k_merkle_verify_proofs"):
            ctx.kernel_timing_read(k)
        got = H.proof_ops_verify(ctx, items)
        assert ctx.kernel_timing_read("k_merkle_value_ops")[1] == 2
        assert got == [C.expected(marks[k]) if k in marks else None for k in range(n)]
        assert H.tx_proofs_validate(ctx, txs * reps) == tx_want * reps
        assert ctx.kernel_timing_read("k_merkle_verify_proofs")[1] == 2
    finally:
        _timing_off(ctx)


def _launches(ctx, items):
    ctx.kernel_timing_read("k_merkle_value_ops")
    got = H.proof_ops_verify(ctx, items)
    return got, ctx.kernel_timing_read("k_merkle_value_ops")[1]


def test_bytes_per_op_rule(ctx, monkeypatch):
    """TMV_DEVICE_PROOF_OPS_MAX_BYTES: values and keys of at most 1,044 bytes per op (the default) still go to
    the device, one byte more does not; the knob moves the edge; an item with a long key stays on the host
    inside a call that goes to the device."""
    monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MIN", "0")
    monkeypatch.delenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES", raising=False)
    gen = P.proofs_from_byte_slices
    key = b"k" * 20

    def item(value_len, key=key):
        return SM.nested([({key: bytes(value_len), b"other": b"v"}, key)], gen)

    at, over = item(1024), item(1025)                               # with the 20-byte key: 1,044 and 1,045
    txs = C.tx_cases()
    ctx.kernel_timing(True)
    try:
        assert _launches(ctx, [at]) == ([None], 1)
        assert _launches(ctx, [over]) == ([None], 0)
        assert _launches(ctx, [at, over]) == ([None, None], 0)      # the call's average decides
        assert _launches(ctx, [at, over, at, item(8)]) == ([None] * 4, 1)
        monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES", "1045")
        assert _launches(ctx, [over]) == ([None], 1)
        monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES", "0")
        empty = item(0, key=b"")
        empty.keys = []                                                # an empty op key consumes no key
        assert _launches(ctx, [empty]) == ([None], 1)                  # nothing to stage at all
        assert _launches(ctx, [item(1)]) == ([None], 0)
        # 64 bytes per op: nine small items carry the average; the item with a 100-byte key is hashed on the
        # host (its lane would read the key byte by byte), the one with a 5,000-byte value too (64 x 64 = 4,096)
        monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES", "64")
        long_key, long_value = item(8, key=b"q" * 100), item(5000)
        bad = SM.nested([({b"q" * 100: b"v", b"other": b"v"}, b"q" * 100)], gen)
        bad.value = b"w"
        got, n = _launches(ctx, [item(8)] * 9 + [long_key, bad])
        assert n == 1 and got[:10] == [None] * 10 and got[10].startswith("leaf hash mismatch: want ")
        assert got[10] == C.expected(bad)
        got, n = _launches(ctx, [item(8)] * 200 + [long_value])
        assert n == 1 and got == [None] * 201
        # tx proofs: the same knob over the txs' bytes
        ctx.kernel_timing_read("k_merkle_verify_proofs")
        ok_tx = txs[1][1]                                              # a 250-byte tx
        assert H.tx_proofs_validate(ctx, [ok_tx]) == [None]
        assert ctx.kernel_timing_read("k_merkle_verify_proofs")[1] == 0
        monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES", "250")
        assert H.tx_proofs_validate(ctx, [ok_tx]) == [None]
        assert ctx.kernel_timing_read("k_merkle_verify_proofs")[1] == 1
    finally:
        _timing_off(ctx)
