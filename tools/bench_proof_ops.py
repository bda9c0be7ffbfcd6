#!/usr/bin/env python3
"""Measurements behind TMV_DEVICE_PROOF_OPS_MIN: the
device path and the host path of tmv_proof_ops_verify and
tmv_tx_proofs_validate, alternating in one session.

  proof_ops   1 and 2 ops per item; values of 32 B, 1 KiB and 64 KiB; 20-byte
              keys; maps of 1,000 pairs; 1 to 100,000 items per call (fewer
              where the values of one call would pass 512 MiB).
              TMV_DEVICE_PROOF_OPS_MAX_BYTES is set out of reach, so the
              threshold alone picks the path and the long values are timed on
              the device too
  tx_proofs   250-byte txs in trees of 100 and 10,000 txs, 1 to 100,000 items

Every figure is the median of --reps calls after one warm-up, with min and
max.  "device" is the call with the threshold at 0 (staging, both kernels and
the host-side sequencing included), "host" the same call with the threshold
out of reach; "kernels" are the device runs' kernel times from
tmv_kernel_timing, so the difference to "device" is what staging costs.  The
C arrays are built once per shape and are not part of any figure.

  python tools/bench_proof_ops.py --out profiles/proof_ops/bench.json [--quick]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native, host as H  # noqa: E402
from tendermint_amd.testing import simple_map as SM  # noqa: E402

KNOB = "TMV_DEVICE_PROOF_OPS_MIN"
BYTES_KNOB = "TMV_DEVICE_PROOF_OPS_MAX_BYTES"  # set out of reach: the threshold alone picks the path here
NEVER = str(0xffffffff)
COUNTS = (1, 10, 100, 1000, 10000, 100000)
MAX_VALUE_BYTES = 512 << 20


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def alternate(ctx, call, kernels, reps):
    """device / host / device / host ...: wall times of both and the device runs' kernel times."""
    wall = {"0": [], NEVER: []}
    kern = {k: [] for k in kernels}
    os.environ[BYTES_KNOB] = str(1 << 24)
    for knob in ("0", NEVER):  # warm-up of both paths
        os.environ[KNOB] = knob
        assert call() == 0
    for k in kernels:
        ctx.kernel_timing_read(k)
    for _ in range(reps):
        for knob in ("0", NEVER):
            os.environ[KNOB] = knob
            t0 = time.perf_counter()
            call()
            wall[knob].append((time.perf_counter() - t0) * 1e3)
            got = {k: ctx.kernel_timing_read(k) for k in kernels}
            if knob == "0":
                assert all(g[1] >= 1 for g in got.values()), "the device path did not launch"
                for k in kernels:
                    kern[k].append(got[k][0])
            else:
                assert all(g[1] == 0 for g in got.values()), "the host path launched a kernel"
    os.environ.pop(KNOB)
    os.environ.pop(BYTES_KNOB)
    return stats(wall["0"]), stats(wall[NEVER]), {k: stats(v) for k, v in kern.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/proof_ops/bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes only (rehearsal)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_proof_ops.py needs a GPU"
    ctx = _native.Context(1)
    ctx.kernel_timing(True)
    rng = np.random.default_rng(19)
    counts = COUNTS[:4] if a.quick else COUNTS
    res = {"device": torch.cuda.get_device_name(0), "library": _native.version(), "reps": a.reps,
           "host_threads": os.environ.get("TMV_HOST_THREADS", "default"), "proof_ops": [], "tx_proofs": []}
    pairs_n = 1000
    for value_bytes in (32, 1024, 65536):
        store = {b"acc/%016d" % i: rng.integers(0, 256, value_bytes, dtype=np.uint8).tobytes() for i in range(pairs_n)}
        inner = SM.SimpleMap(store)
        multi = {b"mod/%016d" % i: rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for i in range(pairs_n - 1)}
        multi[b"store/%014d" % 0] = inner.root
        outer = SM.SimpleMap(multi)
        for n_ops in (1, 2):
            top = min(counts[-1], MAX_VALUE_BYTES // value_bytes)
            items = []
            for i in range(top):
                key = inner.keys[i % pairs_n]
                ops = [inner.op(key)] + ([outer.op(b"store/%014d" % 0)] if n_ops == 2 else [])
                items.append(H.ProofOpsItem(ops, outer.root if n_ops == 2 else inner.root,
                                            ([b"store/%014d" % 0] if n_ops == 2 else []) + [key], store[key]))
            prep = H.PreparedProofOps(items)
            for n in sorted({min(c, top) for c in counts}):
                dev, host, kern = alternate(ctx, lambda: prep.call(ctx, n=n), ("k_merkle_digests_long", "k_merkle_value_ops"),
                                            a.reps)
                row = {"ops_per_item": n_ops, "value_bytes": value_bytes, "key_bytes": 20, "pairs_per_map": pairs_n,
                       "items": n, "ops": n * n_ops, "device": dev, "host": host, "kernels": kern,
                       "device_over_host": round(dev["median_ms"] / host["median_ms"], 3)}
                if value_bytes + 20 > 1044:
                    row["note"] = "above the default of TMV_DEVICE_PROOF_OPS_MAX_BYTES: on the host unless that knob is raised"
                res["proof_ops"].append(row)
                print(json.dumps(row), flush=True)
            del prep, items
    for tree in (100, 10000):
        txs = [rng.integers(0, 256, 250, dtype=np.uint8).tobytes() for _ in range(tree)]
        root, proofs = SM.hashlib_proofs([hashlib.sha256(t).digest() for t in txs])
        top = counts[-1]
        prep = H.PreparedTxProofs([H.TxProof(root, txs[i % tree], proofs[i % tree], root) for i in range(top)])
        for n in counts:
            dev, host, kern = alternate(ctx, lambda: prep.call(ctx, n=n), ("k_merkle_leaves_long", "k_merkle_verify_proofs"),
                                        a.reps)
            row = {"tx_bytes": 250, "txs_per_tree": tree, "items": n, "device": dev, "host": host, "kernels": kern,
                   "device_over_host": round(dev["median_ms"] / host["median_ms"], 3)}
            res["tx_proofs"].append(row)
            print(json.dumps(row), flush=True)
        del prep
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
