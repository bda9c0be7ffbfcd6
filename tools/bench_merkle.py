#!/usr/bin/env python3
"""Measurements behind the merkle proof path (DESIGN.md "Merkle proofs"):

  crossover   k_merkle_leaves_long against k_merkle_leaves (the leaf kernel of
              tmv_merkle_roots, unchanged by the proof work, so it stands for
              the parent's) per leaf length, kernels only, alternating
  lpw         leaves per wave {8, 16, 32, 64} and the shipped rule at 256 to
              21,504 leaves of 64 KiB and up to 65,536 of 16 KiB
  part_sets   part-set headers (roots + leaf hashes, no aunts) of windows of
              1 to 64 x 1 MiB (where the host / device threshold lies),
              100 x 1 MiB and 64 x 21 MiB blocks at 64 KiB parts:
              kernels only, end to end from host buffers, tmv_merkle_roots end
              to end on the same leaves, the host proxy, and the host layer's
              tmv_part_set_headers on its host fallback and on its device path
  verify      Proof.Verify of 100,000 parts' proofs, leaf hashes given

The host column is hashlib (OpenSSL's SHA-NI code) on 16 threads, labelled
"kind": "proxy": Go's crypto/sha256 cannot be run beside it.  Every engine
figure is the median of --reps calls after one warm-up, with min and max.

  python tools/bench_merkle.py --out profiles/merkle/bench.json [--quick]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native, host as H  # noqa: E402

PART = 65536
MAX_CALL = 1 << 30
KERNELS = ("k_merkle_leaves_long", "k_merkle_leaves", "k_merkle_tree_levels", "k_merkle_aunts",
           "k_merkle_verify_proofs")


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def timed(ctx, fn, reps):
    """Wall and summed kernel time of fn() per call (fn is synchronous)."""
    fn()
    for k in KERNELS:
        ctx.kernel_timing_read(k)
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(sum(ctx.kernel_timing_read(k)[0] for k in KERNELS))
    return stats(wall), stats(kern)


def calls_of(blocks_bytes, part):
    """Engine calls (<= 1 GiB each) for blocks of the given sizes laid out one after the other:
    [(byte lo, byte hi, leaf_off, tree_off)]."""
    out, lo, i = [], 0, 0
    while i < len(blocks_bytes):
        j, size = i, 0
        while j < len(blocks_bytes) and size + blocks_bytes[j] <= MAX_CALL:
            size += blocks_bytes[j]
            j += 1
        leaf_off, tree_off = [0], [0]
        base = 0
        for b in blocks_bytes[i:j]:
            t = (b + part - 1) // part
            leaf_off.extend(base + min(b, (k + 1) * part) for k in range(t))
            tree_off.append(tree_off[-1] + t)
            base += b
        out.append((lo, lo + size, np.array(leaf_off, np.uint32), np.array(tree_off, np.uint32)))
        lo += size
        i = j
    return out


def host_proxy(data, calls, pool):
    """hashlib on the pool's threads: leaf hashes in parallel, the small trees on the caller's thread."""
    def leaf(args):
        lo, hi = args
        h = hashlib.sha256(b"\0")
        h.update(data[lo:hi])  # no copy; the GIL is released while a long leaf is hashed
        return h.digest()
    roots = []
    for lo, _, leaf_off, tree_off in calls:
        spans = [(lo + int(leaf_off[i]), lo + int(leaf_off[i + 1])) for i in range(len(leaf_off) - 1)]
        hs = list(pool.map(leaf, spans, chunksize=max(1, len(spans) // 64)))
        for t in range(len(tree_off) - 1):
            level = hs[int(tree_off[t]):int(tree_off[t + 1])]
            if not level:
                roots.append(hashlib.sha256(b"").digest())
                continue
            while len(level) > 1:
                nxt = [hashlib.sha256(b"\1" + level[k] + level[k + 1]).digest() for k in range(0, len(level) - 1, 2)]
                if len(level) & 1:
                    nxt.append(level[-1])
                level = nxt
            roots.append(level[0])
    return b"".join(roots)


def finish(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/merkle/bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes only (rehearsal)")
    ap.add_argument("--sections", default="crossover,lpw,part_sets,verify")
    ap.add_argument("--lpw-shapes", default="", help="leaves x leaf bytes, comma separated, instead of the lpw section's own")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_merkle.py needs a GPU"
    ctx = _native.Context(1)
    ctx.kernel_timing(True)
    rng = np.random.default_rng(11)
    pool = ThreadPoolExecutor(16)
    res = {"device": torch.cuda.get_device_name(0), "library": _native.version(), "reps": a.reps,
           "part_bytes": PART}
    sections = a.sections.split(",")
    big = 21504 if not a.quick else 512
    data = rng.integers(0, 256, big * PART, dtype=np.uint8)

    def proofs_call(lo, hi, leaf_off, tree_off, flags):
        return ctx.merkle_proofs(data[lo:hi], leaf_off, tree_off, flags=flags, aunts=False)

    # 1. crossover: 16 MiB of leaves of one length, long kernel against k_merkle_leaves, alternating
    res["crossover"] = []
    total = (16 << 20) if not a.quick else (1 << 20)
    for ln in (64, 128, 192, 256, 512, 1024, 4096, 16384, PART) if "crossover" in sections else ():
        n = total // ln
        leaf_off = (np.arange(n + 1, dtype=np.uint64) * ln).astype(np.uint32)
        tree_off = np.array([0, n], np.uint32)
        rows = {"leaf_bytes": ln, "n_leaves": n}
        runs = {"long": [], "short": []}
        for _ in range(2):  # long / short / long / short
            for name, fl in (("long", _native.TMV_MERKLE_LONG_LEAVES), ("short", _native.TMV_MERKLE_SHORT_LEAVES)):
                _, k = timed(ctx, lambda fl=fl: proofs_call(0, total, leaf_off, tree_off, fl), max(3, a.reps // 2))
                runs[name].append(k)
        for name in runs:
            rows[name + "_kernels"] = runs[name]
        res["crossover"].append(rows)
        print(json.dumps(rows), flush=True)

    # 2. leaves per wave
    res["lpw"] = []
    # 21,504 leaves exceed one engine call: 16,384 (1 GiB) + 5,120; the sizes between are swept on their own
    # and more leaves than one call holds at 64 KiB with 16 KiB leaves
    shapes = [(n, PART) for n in (256, 1600, 2048, 3072, 4096, 5120, 8192, 10752, 16384, big)]
    shapes += [(16384, 16384), (32768, 16384), (65536, 16384)]
    if a.quick:
        shapes = [(256, PART), (big, PART)]
    if a.lpw_shapes:
        shapes = [tuple(int(x) for x in sh.split("x")) for sh in a.lpw_shapes.split(",")]
    for n, leaf in shapes if "lpw" in sections else ():
        cl = calls_of([leaf] * n, leaf)
        row = {"n_leaves": n, "leaf_bytes": leaf, "engine_calls": len(cl),
               "leaves_per_call": [len(c[2]) - 1 for c in cl]}
        for lpw in (8, 16, 32, 64):
            w, k = timed(ctx, lambda: [proofs_call(*c, _native.merkle_lpw(lpw)) for c in cl], a.reps)
            row["lpw%d" % lpw] = {"kernels": k, "end_to_end": w}
        w, k = timed(ctx, lambda: [proofs_call(*c, 0) for c in cl], a.reps)
        row["rule"] = {"kernels": k, "end_to_end": w}
        res["lpw"].append(row)
        print(json.dumps(row), flush=True)

    # 3. part-set headers of windows of blocks
    res["part_sets"] = []
    windows = [("1 x 1 MiB", [1 << 20]), ("4 x 1 MiB", [1 << 20] * 4), ("8 x 1 MiB", [1 << 20] * 8),
               ("12 x 1 MiB", [1 << 20] * 12), ("16 x 1 MiB", [1 << 20] * 16), ("24 x 1 MiB", [1 << 20] * 24),
               ("32 x 1 MiB", [1 << 20] * 32), ("48 x 1 MiB", [1 << 20] * 48), ("64 x 1 MiB", [1 << 20] * 64),
               ("100 x 1 MiB", [1 << 20] * 100), ("64 x 21 MiB", [21 << 20] * 64)]
    if a.quick:
        windows = windows[:2]
    if "part_sets" not in sections:
        windows = []
    for name, sizes in windows:
        cl = calls_of(sizes, PART)
        nbytes = sum(sizes)
        w, k = timed(ctx, lambda: [proofs_call(*c, 0) for c in cl], a.reps)
        wr, _ = timed(ctx, lambda: [ctx.merkle_roots(data[c[0]:c[1]], c[2], c[3]) for c in cl], max(3, a.reps // 2))
        want = host_proxy(data, cl, pool)
        got = b"".join(proofs_call(*c, 0)[0].tobytes() for c in cl)
        assert got == want, "device roots differ from hashlib's"
        host = []
        for _ in range(max(3, a.reps // 2)):
            t0 = time.perf_counter()
            host_proxy(data, cl, pool)
            host.append((time.perf_counter() - t0) * 1e3)
        layer = {}
        if nbytes <= (128 << 20):  # the host layer's own two paths (include/tmhost.h) on separate block buffers
            off = np.concatenate([[0], np.cumsum(sizes)])
            blocks = [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(sizes))]
            for key, knob in (("host_layer_fallback", str(1 << 62)), ("host_layer_device", "0")):
                os.environ["TMV_DEVICE_MERKLE_MIN"] = knob
                heads = H.part_set_headers(ctx, blocks, PART)
                assert b"".join(h for _, h in heads) == want
                ts = []
                for _ in range(max(3, a.reps // 2)):
                    t0 = time.perf_counter()
                    H.part_set_headers(ctx, blocks, PART)
                    ts.append((time.perf_counter() - t0) * 1e3)
                layer[key] = stats(ts)
            os.environ.pop("TMV_DEVICE_MERKLE_MIN")
            layer["host_layer_fallback"]["what"] = "tmv_part_set_headers below the threshold: portable C++ SHA-256, host pool"
            layer["host_layer_device"]["what"] = "tmv_part_set_headers above the threshold: concatenation + tmv_merkle_proofs"
        row = {"window": name, "bytes": nbytes, "leaves": sum((s + PART - 1) // PART for s in sizes),
               "engine_calls": len(cl), "kernels": k, "end_to_end": w, "tmv_merkle_roots_end_to_end": wr,
               "host_16_threads": dict(stats(host), kind="proxy", what="hashlib (OpenSSL SHA-NI), 16 threads"),
               "end_to_end_GBps": round(nbytes / w["median_ms"] / 1e6, 3),
               "host_GBps": round(nbytes / statistics.median(host) / 1e6, 3), **layer}
        res["part_sets"].append(row)
        print(json.dumps(row), flush=True)

    if "verify" not in sections:
        return finish(a, res)
    # 4. verification of 100,000 parts' proofs, leaf hashes given (trees of 336 parts: 21 MiB blocks)
    per, want_n = 336, (100000 if not a.quick else 5000)
    n_trees = (want_n + per - 1) // per
    n = n_trees * per
    small = rng.integers(0, 256, 8 * n, dtype=np.uint8)
    leaf_off = (np.arange(n + 1, dtype=np.uint64) * 8).astype(np.uint32)
    tree_off = (np.arange(n_trees + 1, dtype=np.uint64) * per).astype(np.uint32)
    roots, leaves, aoff, aunts = ctx.merkle_proofs(small, leaf_off, tree_off)
    total = np.full(n, per, np.int64)
    index = (np.arange(n) % per).astype(np.int64)
    root_per = np.repeat(roots, per, axis=0)
    sl = slice(0, want_n)

    def verify():
        ok, st, _, _, _ = ctx.merkle_verify_proofs(total[sl], index[sl], leaves[sl], aunts[:int(aoff[want_n])],
                                                   aoff[:want_n + 1], root_per[sl])
        assert ok
    w, k = timed(ctx, verify, a.reps)
    # proxy: the same fold with hashlib, one thread, over 5,000 proofs (Python's loop is part of it)
    sub = 5000
    t0 = time.perf_counter()
    for i in range(sub):
        h, j, size = leaves[i].tobytes(), int(index[i]), per
        for q in range(int(aoff[i]), int(aoff[i + 1])):
            while j == size - 1 and size & 1:
                j >>= 1
                size = (size + 1) >> 1
            au = aunts[q].tobytes()
            h = hashlib.sha256(b"\1" + (au + h if j & 1 else h + au)).digest()
            j >>= 1
            size = (size + 1) >> 1
        assert h == root_per[i].tobytes()
    host_ms = (time.perf_counter() - t0) * 1e3 * want_n / sub
    res["verify"] = {"proofs": want_n, "aunts_per_proof": round(int(aoff[want_n]) / want_n, 2), "kernels": k,
                     "end_to_end": w,
                     "host": {"kind": "proxy", "what": "hashlib fold in a Python loop, one thread, scaled from %d proofs;"
                              " /16 for ideal scaling over 16 threads" % sub, "ms": round(host_ms, 2),
                              "ms_16_threads_ideal": round(host_ms / 16, 2)}}
    print(json.dumps(res["verify"]), flush=True)

    finish(a, res)


if __name__ == "__main__":
    main()
