#!/usr/bin/env python3
"""Measurements behind the block wire path:

  window   a 600-block window at section 16's shape (175 signatures and 20
           transactions of 250 bytes per block), validated
             struct   tmv_blocks_validate_basic + tmv_part_set_headers over
                      C structs built beforehand (the two calls of
                      blocksync_replay_full), and the Python conversion that
                      builds those structs from FullBlocks
             wire     one tmv_blocks_validate_wire call over the blocks' bytes
           each on the device path and on the host fallback, alternating, and
           k_span_leaves alone (kernel timing)
  replay   chains.blocksync_replay_wire over 601 such blocks with real
           signatures beside chains.blocksync_replay_full on the same chain
  long     one transaction of 1 KiB .. 256 KiB in one block of the window, its
           Data.Hash on the device and kept on the host: behind
           TMV_DEVICE_WIRE_MAX_TX

Every figure is the median of --reps calls after one warm-up, with min and max.

  python tools/bench_block_wire.py --out profiles/block_wire/bench.json [--quick]
"""
import argparse
import ctypes
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native, chains, host as H  # noqa: E402
from tendermint_amd.testing.block_wire import encode_block  # noqa: E402
from tendermint_amd.testing.blocks import make_full_chain, txs_hash  # noqa: E402

KNOB, CAP = "TMV_DEVICE_BLOCK_MIN", "TMV_DEVICE_WIRE_MAX_TX"
PART_SIZE = 65536


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


class Wire:
    """One tmv_blocks_validate_wire call over prepared buffers."""

    def __init__(self, ctx, raws):
        self.L = H._setup_block_wire(_native.lib())
        self.ctx, self.w = ctx, H.WireWindow(raws)
        m = max(1, self.w.n)
        self.results, self.reason = (ctypes.c_int32 * m)(), (ctypes.c_int32 * m)()
        self.errs = ctypes.create_string_buffer(H.ERR_STRIDE * m)
        self.hashes, self.has = (ctypes.c_uint8 * (32 * m))(), (ctypes.c_uint8 * m)()
        self.totals, self.phash = (ctypes.c_uint32 * m)(), (ctypes.c_uint8 * (32 * m))()

    def __call__(self):
        rc = self.L.tmv_blocks_validate_wire(self.ctx.handle, ctypes.cast(self.w.data, H._u8p), self.w.off, self.w.n,
                                             PART_SIZE, self.results, self.reason, self.errs, H.ERR_STRIDE,
                                             ctypes.cast(self.hashes, H._u8p), ctypes.cast(self.has, H._u8p),
                                             self.totals, ctypes.cast(self.phash, H._u8p), None)
        assert rc == 0, rc
        return bytes(self.hashes), bytes(self.phash)


class Struct:
    """tmv_blocks_validate_basic + tmv_part_set_headers over prepared structs."""

    def __init__(self, ctx, blocks):
        self.L = H._setup_merkle(H._setup_blocks(_native.lib()))
        self.ctx, self.pb, self.k = ctx, H.PreparedBlocks(blocks), H._Keep()
        n = len(blocks)
        self.arr = (H.CBytes * n)()
        for i, b in enumerate(blocks):
            self.arr[i] = H._ref_bytes(self.k, b.raw)
        self.totals, self.phash = (ctypes.c_uint32 * n)(), (ctypes.c_uint8 * (32 * n))()

    def __call__(self):
        pb = self.pb
        rc = self.L.tmv_blocks_validate_basic(self.ctx.handle, pb.arr, pb.n, pb.results, pb.errs, H.ERR_STRIDE,
                                              ctypes.cast(pb.hashes, H._u8p), ctypes.cast(pb.has, H._u8p))
        assert rc == 0, rc
        rc = self.L.tmv_part_set_headers(self.ctx.handle, self.arr, pb.n, PART_SIZE, self.totals,
                                         ctypes.cast(self.phash, H._u8p))
        assert rc == 0, rc
        return bytes(pb.hashes), bytes(self.phash)


def with_env(fn, **kw):
    def run():
        old = {k: os.environ.get(k) for k in kw}
        os.environ.update({k: str(v) for k, v in kw.items()})
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="60 blocks of 25 signatures, 3 reps")
    a = ap.parse_args()
    n_blocks, n_vals, reps = (60, 25, 3) if a.quick else (600, 175, a.reps)
    ctx = _native.Context(1)
    _, blocks, _ = make_full_chain(n_blocks, n_vals, seed=16, txs=(20, 20), tx_len=(250, 250), sign=False, wire=True)
    raws = [b.raw for b in blocks]
    out = {"shape": {"blocks": n_blocks, "signatures": n_vals, "txs": 20, "tx_len": 250,
                     "bytes": sum(len(r) for r in raws), "part_size": PART_SIZE}, "window": {}, "long": []}

    wire, struct = Wire(ctx, raws), Struct(ctx, blocks)
    assert wire() == struct(), "the two paths disagree"
    off, on = {KNOB: 1 << 30}, {KNOB: 32}
    runs = {"struct_device": with_env(struct, **on), "wire_device": with_env(wire, **on),
            "struct_host": with_env(struct, **off), "wire_host": with_env(wire, **off)}
    ts = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    for _ in range(reps):  # alternating, so that drift hits all four alike
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    out["window"] = {k: stats(v) for k, v in ts.items()}
    out["window"]["python_prepared_blocks"] = stats(wall(lambda: H.PreparedBlocks(blocks), min(reps, 5)))
    out["window"]["python_wire_window"] = stats(wall(lambda: H.WireWindow(raws), min(reps, 5)))
    ctx.kernel_timing(True)
    ctx.kernel_timing_read("k_span_leaves")
    kern = []
    for _ in range(reps):
        runs["wire_device"]()
        ms, launches = ctx.kernel_timing_read("k_span_leaves")
        assert launches == 1
        kern.append(ms)
    ctx.kernel_timing(False)
    out["window"]["k_span_leaves"] = stats(kern)

    for kib in ([1, 16] if a.quick else [1, 2, 4, 16, 64, 256]):
        b = dataclasses.replace(blocks[n_blocks // 2], txs=[b"\x5a" * (kib << 10)] + blocks[n_blocks // 2].txs[1:])
        b = dataclasses.replace(b, header=dataclasses.replace(b.header, data_hash=txs_hash(b.txs)))
        rs = list(raws)
        rs[n_blocks // 2] = encode_block(b)[0]
        w = Wire(ctx, rs)
        dev, host = with_env(w, **{CAP: 1 << 30}), with_env(w, **{CAP: 512})
        assert dev() == host()
        td, th = [], []
        for _ in range(reps):
            for fn, t in ((dev, td), (host, th)):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
        out["long"].append({"tx_kib": kib, "tree_on_device": stats(td), "tree_on_host": stats(th)})

    # the drivers over real signatures: FullBlocks built beforehand against the blocks' bytes
    vals, blocks, _ = make_full_chain(n_blocks + 1, n_vals, seed=4, txs=(20, 20), tx_len=(250, 250), wire=True)
    raws = [b.raw for b in blocks]
    full = lambda: chains.blocksync_replay_full(ctx, "test_chain_id", vals, blocks, H.BlockID())
    wire = lambda: chains.blocksync_replay_wire(ctx, "test_chain_id", vals, raws, H.BlockID())
    assert full() == wire() == (n_blocks, None)
    tf, tw = [], []
    for _ in range(max(3, reps // 3)):  # alternating
        for fn, t in ((full, tf), (wire, tw)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    out["replay"] = {"blocks": n_blocks, "validators": n_vals, "bytes": sum(len(r) for r in raws),
                     "blocksync_replay_full": stats(tf), "blocksync_replay_wire": stats(tw),
                     "what": "both include their Python conversion; the wire driver reads headers and transactions "
                             "out of the views and passes the views' commits to tmv_verify_commits by pointer"}

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
