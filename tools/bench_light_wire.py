#!/usr/bin/env python3
"""Measurements behind the light-block wire path:

  window   600 light blocks at config 3's shape (100 validators, one key
           rotated per height), validated
             wire     one tmv_light_blocks_validate_wire call over the bytes,
                      on the device path and on the host path
             struct   tmv_header_hashes + tmv_validator_set_hashes over C
                      structs and columns built beforehand (the hashes alone:
                      the host layer has no struct form of
                      LightBlock.ValidateBasic)
           alternating in one process, the Python time in front of each, and
           k_valset_span_leaves alone (kernel timing)
  drivers  chains.statesync_backfill over the window, and
           chains.verify_sequential_wire beside chains.verify_sequential on the
           same signed chain
  large    the same columns at 10,000 validators with a smaller window
  sweep    the wire call on both paths at window sizes around
           TMV_DEVICE_HASH_MIN

Every figure is the median of --reps calls after one warm-up, with min and max.

  python tools/bench_light_wire.py --out profiles/light_wire/bench.json [--quick]
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
from tendermint_amd.testing.factory import make_light_chain  # noqa: E402
from tendermint_amd.testing.light_wire import encode_light_block  # noqa: E402

KNOB = "TMV_DEVICE_HASH_MIN"
CHAIN = "test"
PERIOD, DRIFT = 3 * 3600 * 10**9, 10 * 10**9


def note(what):
    print("[bench_light_wire] " + what, file=sys.stderr, flush=True)


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


def alternating(runs, reps):
    ts = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    for _ in range(reps):  # alternating, so that drift hits all alike
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ts.items()}


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


class Wire:
    """One tmv_light_blocks_validate_wire call over prepared buffers."""

    def __init__(self, ctx, raws):
        self.L = H._setup_light_wire(_native.lib())
        self.ctx, self.w = ctx, H.WireWindow(raws)
        m = max(1, self.w.n)
        self.results, self.reason = (ctypes.c_int32 * m)(), (ctypes.c_int32 * m)()
        self.errs = ctypes.create_string_buffer(H.ERR_STRIDE * m)
        self.hashes, self.vhashes, self.has = (ctypes.c_uint8 * (32 * m))(), (ctypes.c_uint8 * (32 * m))(), \
            (ctypes.c_uint8 * m)()

    def __call__(self):
        rc = self.L.tmv_light_blocks_validate_wire(self.ctx.handle, CHAIN.encode(), ctypes.cast(self.w.data, H._u8p),
                                                   self.w.off, self.w.n, self.results, self.reason, self.errs,
                                                   H.ERR_STRIDE, ctypes.cast(self.hashes, H._u8p),
                                                   ctypes.cast(self.has, H._u8p), ctypes.cast(self.vhashes, H._u8p),
                                                   None)
        assert rc == 0, (rc, self.errs.raw[:200])
        return bytes(self.hashes), bytes(self.vhashes)


class Struct:
    """tmv_header_hashes over prepared tmv_header structs + tmv_validator_set_hashes over prepared columns."""

    def __init__(self, ctx, blocks):
        self.L = H._setup_light(H._setup(_native.lib()))
        self.ctx, self.k, n = ctx, H._Keep(), len(blocks)
        self.arr = (H.CHeader * n)()
        for i, b in enumerate(blocks):
            self.arr[i] = H._c_header(self.k, b.signed_header.header)
        self.n = n
        self.out, self.has = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * n)()
        self.cols = chains.validator_set_arrays([b.vals for b in blocks])

    def __call__(self):
        rc = self.L.tmv_header_hashes(self.ctx.handle, self.arr, self.n, ctypes.cast(self.out, H._u8p),
                                      ctypes.cast(self.has, H._u8p))
        assert rc == 0, rc
        return bytes(self.out), self.ctx.validator_set_hashes(*self.cols).tobytes()


def columns(ctx, blocks, raws, reps, out):
    wire, struct = Wire(ctx, raws), Struct(ctx, blocks)
    assert wire() == struct(), "the two paths disagree"
    runs = {"wire_device": with_env(wire, **{KNOB: 1}), "wire_host": with_env(wire, **{KNOB: 1 << 30}),
            "struct_device": struct}
    assert runs["wire_device"]() == runs["wire_host"]()
    out.update(alternating(runs, reps))
    out["python_wire_window"] = stats(wall(lambda: H.WireWindow(raws), reps))
    out["python_structs_and_columns"] = stats(wall(lambda: Struct(ctx, blocks), reps))
    ctx.kernel_timing(True)
    ctx.kernel_timing_read("k_valset_span_leaves")
    kern = []
    for _ in range(reps):
        runs["wire_device"]()
        ms, launches = ctx.kernel_timing_read("k_valset_span_leaves")
        assert launches == 1
        kern.append(ms)
    ctx.kernel_timing(False)
    ctx.kernel_timing_read("k_span_leaves")
    out["k_valset_span_leaves"] = stats(kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="60 light blocks of 10 validators, 3 reps")
    a = ap.parse_args()
    n_blocks, n_vals, reps = (60, 10, 3) if a.quick else (600, 100, a.reps)
    big_blocks, big_vals = (4, 500) if a.quick else (16, 10_000)
    ctx = _native.Context(1)
    trusted, blocks = make_light_chain(n_blocks, n_vals, CHAIN)
    raws = [encode_light_block(b)[0] for b in blocks]
    note("chain made")
    out = {"shape": {"light_blocks": n_blocks, "validators": n_vals, "bytes": sum(len(r) for r in raws)}, "window": {}}
    columns(ctx, blocks, raws, reps, out["window"])

    note("window done")
    # the drivers: newest first for backfill; real signatures for the light client
    top = blocks[-1].signed_header.commit.block_id.hash
    newest = raws[::-1]
    backfill = lambda: chains.statesync_backfill(ctx, CHAIN, newest, top, window=n_blocks)  # noqa: E731
    assert backfill()[:2] == (n_blocks, None)
    now = (blocks[-1].signed_header.header.time[0] + 5, 0)
    seq = lambda: chains.verify_sequential(ctx, trusted, blocks, PERIOD, now, DRIFT, window=n_blocks)  # noqa: E731
    seqw = lambda: chains.verify_sequential_wire(ctx, trusted, raws, PERIOD, now, DRIFT, window=n_blocks)  # noqa: E731
    assert seq() == seqw() == (n_blocks, None)
    out["drivers"] = alternating({"statesync_backfill": backfill, "verify_sequential": seq,
                                  "verify_sequential_wire": seqw}, reps)
    out["drivers"]["what"] = ("all include their Python conversion; verify_sequential_wire makes one wire call per "
                              "window for the views and passes them to tmv_light_verify_many by pointer, which "
                              "hashes headers and sets again on its own path")

    note("drivers done")
    # 10,000 validators: the signatures are not read by either column, so one set and its commit are reused
    _, (one,) = make_light_chain(1, big_vals, CHAIN, seed=3)
    big = [dataclasses.replace(one) for _ in range(big_blocks)]
    braws = [encode_light_block(one)[0]] * big_blocks
    out["large"] = {"shape": {"light_blocks": big_blocks, "validators": big_vals, "bytes": sum(len(r) for r in braws)}}
    columns(ctx, big, braws, reps, out["large"])

    note("large done")
    # the threshold: both paths at window sizes around TMV_DEVICE_HASH_MIN
    out["sweep"] = []
    for m in ([8, 32] if a.quick else [4, 8, 16, 24, 32, 48, 64, 128]):
        w = Wire(ctx, raws[:m])
        r = alternating({"wire_device": with_env(w, **{KNOB: 1}), "wire_host": with_env(w, **{KNOB: 1 << 30})}, reps)
        out["sweep"].append({"light_blocks": m, "validators": n_vals, **r})

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
