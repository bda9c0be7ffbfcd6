#!/usr/bin/env python3
"""Measurements behind the results hash:

  engine      tmv_tx_results_hashes over 600 blocks' results from host columns,
              end to end, and k_result_leaves alone (kernel timing), at data of
              0 and 100 bytes per result
  host_layer  tmv_results_hash_many over C structs of the same shapes, on its
              host fallback and on its device path, alternating
  sweep       results per call 64 .. 400,000 (blocks of 200 results), fallback
              and device path alternating in one session, at data 0 and 100:
              behind TMV_DEVICE_RESULTS_MIN -- the threshold of a shape is the
              smallest count from which the device path stays ahead
  long        one result of 1 KiB .. 1 MiB inside a 100,000-result call, with
              its tree on the device and kept on the host: behind
              TMV_DEVICE_RESULTS_MAX_DATA

Every figure is the median of --reps calls after one warm-up, with min and max.

  python tools/bench_results.py --out profiles/results_hash/bench.json [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native, host as H  # noqa: E402
from tendermint_amd.testing.blocks import results_hash  # noqa: E402

PER_BLOCK = 200
KNOB, CAP = "TMV_DEVICE_RESULTS_MIN", "TMV_DEVICE_RESULTS_MAX_DATA"
R = H.CTxResult
DT = np.dtype({"names": ["code", "data_p", "data_len", "gas_wanted", "gas_used"],
               "formats": [np.uint32, np.uint64, np.uint32, np.int64, np.int64],
               "offsets": [R.code.offset, R.data.offset + H.CBytes.p.offset, R.data.offset + H.CBytes.len.offset,
                           R.gas_wanted.offset, R.gas_used.offset], "itemsize": ctypes.sizeof(R)})


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


class Results:
    """n results in trees of `per` (the last one shorter) as column arrays and
    as C structs over the same memory; lens: the data length of each."""

    def __init__(self, lens, rng, per=PER_BLOCK):
        n = len(lens)
        self.n = n
        self.code = np.where(rng.integers(0, 10, n) == 0, rng.integers(1, 1 << 20, n), 0).astype(np.uint32)
        self.gw = rng.integers(0, 1 << 22, n).astype(np.int64)
        self.gu = rng.integers(0, 1 << 22, n).astype(np.int64)
        self.data_off = np.zeros(n + 1, np.uint32)
        self.data_off[1:] = np.cumsum(lens)
        self.data = rng.integers(0, 256, max(int(self.data_off[-1]), 1), dtype=np.uint8)
        self.tree_off = np.append(np.arange(0, n, per), n).astype(np.uint32)
        self.n_trees = len(self.tree_off) - 1
        s = np.zeros(n, DT)
        s["code"], s["gas_wanted"], s["gas_used"], s["data_len"] = self.code, self.gw, self.gu, lens
        s["data_p"] = np.where(np.asarray(lens) > 0, self.data.ctypes.data + self.data_off[:-1].astype(np.uint64), 0)
        self.c = s
        self.ptrs = (ctypes.POINTER(R) * self.n_trees)()
        self.counts = (ctypes.c_uint32 * self.n_trees)()
        for t in range(self.n_trees):
            self.ptrs[t] = ctypes.cast(s.ctypes.data + DT.itemsize * int(self.tree_off[t]), ctypes.POINTER(R))
            self.counts[t] = int(self.tree_off[t + 1] - self.tree_off[t])
        self.out = np.zeros(32 * self.n_trees, np.uint8)

    def columns(self):
        return self.code, self.gw, self.gu, self.data, self.data_off, self.tree_off

    def layer(self, L, ctx):
        rc = L.tmv_results_hash_many(ctx.handle, self.ptrs, self.counts, None, self.n_trees,
                                     ctypes.cast(self.out.ctypes.data, H._u8p))
        assert rc == 0, rc
        return self.out.tobytes()

    def want(self):
        d = self.data.tobytes()
        rs = [H.TxResult(int(self.code[i]), d[self.data_off[i]:self.data_off[i + 1]], int(self.gw[i]), int(self.gu[i]))
              for i in range(self.n)]
        return b"".join(results_hash(rs[self.tree_off[t]:self.tree_off[t + 1]]) for t in range(self.n_trees))


def alternate(L, ctx, rs, reps, rounds=2, env=None):
    """The host layer's fallback and device path, alternating: {"fallback": [...], "device": [...]} in ms."""
    runs = {"fallback": [], "device": []}
    for _ in range(rounds):
        for key, knob in (("fallback", str(1 << 40)), ("device", "1")):
            os.environ[KNOB] = knob
            runs[key] += wall(lambda: rs.layer(L, ctx), reps)
    os.environ.pop(KNOB)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/results_hash/bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes only (rehearsal)")
    ap.add_argument("--sections", default="engine,host_layer,sweep,long")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_results.py needs a GPU"
    ctx = _native.Context(1)
    ctx.kernel_timing(True)
    L = H._setup_results(_native.lib())
    rng = np.random.default_rng(21)
    res = {"device": torch.cuda.get_device_name(0), "library": _native.version(), "reps": a.reps,
           "results_per_block": PER_BLOCK}
    sections = a.sections.split(",")
    big = 600 * PER_BLOCK if not a.quick else 20 * PER_BLOCK

    def shape(n, nbytes):
        return Results(np.full(n, nbytes, np.uint32), rng)

    # 1. / 2. a 600-block window: the engine call and the host layer on both paths
    res["window"] = []
    if "engine" in sections or "host_layer" in sections:
        for nbytes in (0, 100):
            rs = shape(big, nbytes)
            want = rs.want()
            assert ctx.tx_results_hashes(*rs.columns()).tobytes() == want, "engine roots differ from hashlib's"
            row = {"results": big, "trees": rs.n_trees, "data_bytes": nbytes}
            if "engine" in sections:
                ctx.kernel_timing_read("k_result_leaves")
                eng, kern = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ctx.tx_results_hashes(*rs.columns())
                    eng.append((time.perf_counter() - t0) * 1e3)
                    kern.append(ctx.kernel_timing_read("k_result_leaves")[0])
                row["engine_end_to_end"], row["k_result_leaves"] = stats(eng), stats(kern)
            if "host_layer" in sections:
                for key, knob in (("fallback", str(1 << 40)), ("device", "1")):
                    os.environ[KNOB] = knob
                    assert rs.layer(L, ctx) == want, key
                runs = alternate(L, ctx, rs, max(3, a.reps // 2))
                row["host_layer_fallback"], row["host_layer_device"] = stats(runs["fallback"]), stats(runs["device"])
            res["window"].append(row)
            print(json.dumps(row), flush=True)

    # 3. the threshold: results per call, both paths alternating, at data 0 and 100
    res["sweep"] = []
    if "sweep" in sections:
        res["sweep_threshold"] = {}
        counts = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 400000)
        for nbytes in (0, 100):
            rows = []
            for n in counts:
                if a.quick and n > 8192:
                    break
                rs = shape(n, nbytes)
                runs = alternate(L, ctx, rs, a.reps)
                row = {"data_bytes": nbytes, "results": n, "fallback": stats(runs["fallback"]),
                       "device": stats(runs["device"])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            res["sweep"] += rows
            slower = [r["results"] for r in rows if r["device"]["median_ms"] > r["fallback"]["median_ms"]]
            res["sweep_threshold"][str(nbytes)] = min((r["results"] for r in rows
                                                       if not slower or r["results"] > max(slower)), default=None)
        print("threshold", res["sweep_threshold"], flush=True)

    # 4. one long result inside a large call: its tree on the device, and kept on the host by the cap
    res["long"] = []
    if "long" in sections:
        n = 100000 if not a.quick else 4000
        for long_bytes in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20):
            lens = np.full(n, 100, np.uint32)
            lens[n // 2] = long_bytes
            rs = Results(lens, rng)
            row = {"results": n, "long_bytes": long_bytes}
            os.environ[KNOB] = "1"
            for key, cap in (("tree_on_device", str(1 << 30)), ("tree_on_host", str(long_bytes - 1))):
                os.environ[CAP] = cap
                row[key] = stats(wall(lambda: rs.layer(L, ctx), a.reps))
            os.environ.pop(CAP)
            os.environ.pop(KNOB)
            res["long"].append(row)
            print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
