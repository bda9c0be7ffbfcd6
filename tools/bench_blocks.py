#!/usr/bin/env python3
"""Measurements behind the block validation path (DESIGN.md "Block validation"):

  commit_hash  Commit.Hash of 600 and 10,000 commits of 175 signatures:
               the engine call from host columns end to end (and its kernels),
               the host layer on its host fallback and on its device path
               (tmv_commit_hash_many over C structs), and a 16-thread hashlib
               proxy over pre-encoded leaves
  sweep        commits per call 1 .. 600, of 175 and of 7 signatures: the host
               layer's fallback against its device path, alternating; the
               threshold of a shape is the smallest count from which the device
               path is no slower
  validate     tmv_blocks_validate_basic of a 600-block window (175 signatures,
               20 transactions of 250 bytes per block), both paths
  replay       chains.blocksync_replay_full over 601 blocks of 175 validators
               with real signatures, beside chains.blocksync_replay (the commit
               checks alone, BlockIDs taken from the caller) on the same chain

The proxy is hashlib (OpenSSL's SHA-NI code), labelled "kind": "proxy": Go's
crypto/sha256 cannot be run beside it, and Python holds the GIL while it hashes
a 110-byte leaf, so its 16 threads add little.  Every figure is the median of
--reps calls after one warm-up, with min and max.

  python tools/bench_blocks.py --out profiles/block_validate/bench.json [--quick]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native, chains, host as H  # noqa: E402
from tendermint_amd.testing.blocks import commit_sig_bytes, make_full_chain  # noqa: E402

SIGS = 175
T0 = 1577836800
KNOB = "TMV_DEVICE_BLOCK_MIN"


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


class Commits:
    """n commits of SIGS signatures (one absent in 16) as column arrays, as C
    structs over the same memory, and as pre-encoded leaves."""

    def __init__(self, n, rng, sigs=SIGS):
        m = n * sigs
        self.n, self.sigs = n, sigs
        absent = rng.integers(0, 16, m) == 0
        self.flag = np.where(absent, 1, 2).astype(np.uint8)
        self.addr_len = np.where(absent, 0, 20).astype(np.uint8)
        self.addr = rng.integers(0, 256, (m, 20), dtype=np.uint8)
        self.secs = np.where(absent, -62135596800, T0 + np.arange(m) // sigs).astype(np.int64)
        self.nanos = np.where(absent, 0, rng.integers(0, 10**9, m)).astype(np.int32)
        self.sig_len = np.where(absent, 0, 64).astype(np.uint8)
        self.sig = rng.integers(0, 256, (m, 64), dtype=np.uint8)
        self.off = (np.arange(n + 1, dtype=np.uint64) * sigs).astype(np.uint32)
        s = np.zeros(m, H._dt("s", H.CCommitSig))
        s["block_id_flag"] = self.flag
        s["validator_address"] = np.where(absent, 0, self.addr.ctypes.data + 20 * np.arange(m, dtype=np.uint64))
        s["validator_address_len"] = self.addr_len
        s["ts_seconds"], s["ts_nanos"] = self.secs, self.nanos
        s["signature"] = np.where(absent, 0, self.sig.ctypes.data + 64 * np.arange(m, dtype=np.uint64))
        s["signature_len"] = self.sig_len
        self.c_sigs = s
        self.c_commits = (H.CCommit * n)()
        self.c_ptrs = (ctypes.POINTER(H.CCommit) * n)()
        stride = ctypes.sizeof(H.CCommitSig)
        for c in range(n):
            self.c_commits[c].height = c + 1
            self.c_commits[c].sigs = ctypes.cast(s.ctypes.data + stride * sigs * c, ctypes.POINTER(H.CCommitSig))
            self.c_commits[c].n_sigs = sigs
            self.c_ptrs[c] = ctypes.pointer(self.c_commits[c])

    def columns(self, n=None):
        n = self.n if n is None else n
        m = n * self.sigs
        return (self.flag[:m], self.addr_len[:m], self.addr[:m], self.secs[:m], self.nanos[:m], self.sig_len[:m],
                self.sig[:m], self.off[:n + 1])

    def leaves(self):
        addr, sig = self.addr.tobytes(), self.sig.tobytes()
        out = []
        for i in range(self.n * self.sigs):
            al, sl = int(self.addr_len[i]), int(self.sig_len[i])
            out.append(b"\0" + commit_sig_bytes(H.CommitSig(int(self.flag[i]), addr[20 * i:20 * i + al],
                                                             (int(self.secs[i]), int(self.nanos[i])),
                                                             sig[64 * i:64 * i + sl])))
        return out


def layer_call(L, ctx, cm, n, out):
    rc = L.tmv_commit_hash_many(ctx.handle, cm.c_ptrs, n, ctypes.cast(out.ctypes.data, H._u8p), None)
    assert rc == 0, rc


def proxy_roots(leaves, n, pool):
    def one(c):
        level = [hashlib.sha256(x).digest() for x in leaves[c * SIGS:(c + 1) * SIGS]]
        while len(level) > 1:
            nxt = [hashlib.sha256(b"\1" + level[k] + level[k + 1]).digest() for k in range(0, len(level) - 1, 2)]
            if len(level) & 1:
                nxt.append(level[-1])
            level = nxt
        return level[0]
    return b"".join(pool.map(one, range(n), chunksize=max(1, n // 64)))


def finish(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/block_validate/bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes only (rehearsal)")
    ap.add_argument("--sections", default="commit_hash,sweep,validate,replay")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_blocks.py needs a GPU"
    ctx = _native.Context(1)
    ctx.kernel_timing(True)
    L = H._setup_blocks(_native.lib())
    rng = np.random.default_rng(17)
    pool = ThreadPoolExecutor(16)
    res = {"device": torch.cuda.get_device_name(0), "library": _native.version(), "reps": a.reps,
           "signatures_per_commit": SIGS}
    sections = a.sections.split(",")
    sizes = (600, 10000) if not a.quick else (40, 200)
    cm = Commits(max(sizes), rng)

    # 1. Commit.Hash of 600 and 10,000 commits
    res["commit_hash"] = []
    if "commit_hash" in sections:
        leaves = cm.leaves()
        for n in sizes:
            want = proxy_roots(leaves, n, pool)
            cols = cm.columns(n)
            assert ctx.commit_hashes(*cols).tobytes() == want, "engine roots differ from hashlib's"
            ctx.kernel_timing_read("k_commit_leaves")
            eng, kern = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.commit_hashes(*cols)
                eng.append((time.perf_counter() - t0) * 1e3)
                kern.append(ctx.kernel_timing_read("k_commit_leaves")[0])
            out = np.zeros(32 * n, np.uint8)
            row = {"commits": n, "leaves": n * SIGS, "engine_end_to_end": stats(eng),
                   "k_commit_leaves": stats(kern)}
            for key, knob in (("host_layer_fallback", str(1 << 31)), ("host_layer_device", "0")):
                os.environ[KNOB] = knob
                layer_call(L, ctx, cm, n, out)
                assert out.tobytes() == want, key
                row[key] = stats(wall(lambda: layer_call(L, ctx, cm, n, out), max(3, a.reps // 2)))
            os.environ.pop(KNOB)
            row["host_layer_fallback"]["what"] = "tmv_commit_hash_many below the threshold: portable C++ SHA-256, host pool"
            row["host_layer_device"]["what"] = "tmv_commit_hash_many above the threshold: columns packed + tmv_commit_hashes"
            row["host_16_threads"] = dict(stats(wall(lambda: proxy_roots(leaves, n, pool), 3)), kind="proxy",
                                          what="hashlib (OpenSSL SHA-NI) over pre-encoded leaves, 16 threads")
            res["commit_hash"].append(row)
            print(json.dumps(row), flush=True)

    # 2. the threshold: commits per call, fallback and device path alternating, at config 4's 175
    # signatures per commit and at a small validator set's 7
    res["sweep"] = []
    if "sweep" in sections:
        res["sweep_threshold"] = {}
        for sigs in (SIGS, 7):
            cs = cm if sigs == SIGS else Commits(600, rng, sigs)
            rows = []
            for n in (1, 2, 4, 8, 16, 24, 32, 48, 64, 128, 256, 600):
                if n > cs.n:
                    break
                out = np.zeros(32 * n, np.uint8)
                runs = {"fallback": [], "device": []}
                for _ in range(2):
                    for key, knob in (("fallback", str(1 << 31)), ("device", "0")):
                        os.environ[KNOB] = knob
                        runs[key] += wall(lambda: layer_call(L, ctx, cs, n, out), a.reps)
                os.environ.pop(KNOB)
                row = {"signatures_per_commit": sigs, "commits": n, "fallback": stats(runs["fallback"]),
                       "device": stats(runs["device"])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            res["sweep"] += rows
            slower = [r["commits"] for r in rows if r["device"]["median_ms"] > r["fallback"]["median_ms"]]
            res["sweep_threshold"][str(sigs)] = min((r["commits"] for r in rows
                                                     if not slower or r["commits"] > max(slower)), default=None)
        print("threshold", res["sweep_threshold"], flush=True)

    # 3. Block.ValidateBasic of a 600-block window
    n_blocks = 600 if not a.quick else 40
    if "validate" in sections:
        _, blocks, _ = make_full_chain(n_blocks + 1, SIGS, seed=3, raw_len=(1, 2), txs=(20, 20), tx_len=(250, 250),
                                       sign=False)
        pb = H.PreparedBlocks(blocks[1:])
        row = {"blocks": n_blocks, "txs_per_block": 20, "tx_bytes": 250}
        for key, knob in (("host_fallback", str(1 << 31)), ("device", "0")):
            os.environ[KNOB] = knob
            assert all(e is None for e, _ in pb.run(ctx)), key
            row[key] = stats(wall(lambda: pb.run(ctx), a.reps))
        os.environ.pop(KNOB)
        res["validate"] = row
        print(json.dumps(row), flush=True)

    # 4. the replay driver over real signatures
    if "replay" in sections:
        vals, blocks, ids = make_full_chain(n_blocks + 1, SIGS, seed=4, raw_len=(20000, 200000), txs=(20, 20),
                                            tx_len=(250, 250))
        light = [chains.Block(b.height, i, b.last_commit) for b, i in zip(blocks, ids)]
        light[0].last_commit = None
        row = {"blocks": n_blocks, "validators": SIGS, "raw_bytes": sum(len(b.raw) for b in blocks)}
        assert chains.blocksync_replay_full(ctx, "test_chain_id", vals, blocks, H.BlockID()) == (n_blocks, None)
        assert chains.blocksync_replay(ctx, "test_chain_id", vals, light, H.BlockID()) == (n_blocks, None)
        runs = {"blocksync_replay_full": [], "blocksync_replay": []}
        for _ in range(max(3, a.reps // 2)):  # alternating
            t0 = time.perf_counter()
            chains.blocksync_replay_full(ctx, "test_chain_id", vals, blocks, H.BlockID())
            runs["blocksync_replay_full"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            chains.blocksync_replay(ctx, "test_chain_id", vals, light, H.BlockID())
            runs["blocksync_replay"].append((time.perf_counter() - t0) * 1e3)
        for k, v in runs.items():
            row[k] = stats(v)
        row["blocksync_replay"]["what"] = "the commit checks alone, BlockIDs taken from the caller (Python conversion included)"
        row["blocksync_replay_full"]["what"] = "BlockIDs derived, Block.ValidateBasic and the header checks added (Python conversion included)"
        res["replay"] = row
        print(json.dumps(row), flush=True)

    finish(a, res)


if __name__ == "__main__":
    main()
