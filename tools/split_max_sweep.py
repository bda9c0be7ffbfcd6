#!/usr/bin/env python3
"""Sweep of the split's leader threshold (split.h, MsmParams::split_max).

One tmv_verify_batches_device launch of K C2 batches of one validator set is
one tile of the column order, so a group of 128 slots holds 128 / K leaders:
K = 32, 16 and 8 put 4, 8 and 16 leaders into every group.  Each launch is
timed alone (HIP events, one launch at a time) with the split off and forced on
(test aid split_groups) with split_max = 4, 8 and 16, and the device's
count of split groups and high points is printed beside the time:

  python tools/split_max_sweep.py [--batch 10000] [--reps 20]
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from tendermint_amd import _native as N  # noqa: E402
from tendermint_amd.testing.factory import make_c2_batch  # noqa: E402


def option(name, v):
    L = N.lib()
    L.tmv_internal_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    assert L.tmv_internal_option(name, int(v)) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiles", default="32,16,8")
    ap.add_argument("--values", default="0,4,8,16", help="split_max values; 0 = the split off")
    args = ap.parse_args()
    tiles = [int(x) for x in args.tiles.split(",")]
    dev = torch.device("cuda:0")
    ctx = N.Context(1)
    ctx.set_batch_options(group_log2=7, window_bits=5, stats=True)
    n = args.batch
    d_in = []
    for j in range(min(max(tiles), 64)):  # (more batches cycle through 64 resident ones, as the benchmark's do)
        b = make_c2_batch(n, seed=0xED25519 + j)
        d_in.append((torch.from_numpy(b.pk).to(dev), torch.from_numpy(b.sig).to(dev), torch.from_numpy(b.msg).to(dev),
                     torch.from_numpy(b.off.view("int32")).to(dev), int(b.off[-1] - b.off[0])))
    out = torch.zeros(max(tiles) * n, dtype=torch.int8, device=dev)
    st = torch.cuda.Stream(dev)  # a stream of its own: the events below bracket the launch's kernels
    stream = st.cuda_stream
    try:
        for K in tiles:
            refs = [N.BatchRef(pk.data_ptr(), sig.data_ptr(), msg.data_ptr(), off.data_ptr(), n, mb,
                               out[j * n:(j + 1) * n].data_ptr()) for j, (pk, sig, msg, off, mb) in enumerate(d_in[j % len(d_in)] for j in range(K))]
            for v in (int(x) for x in args.values.split(",")):
                option(b"split_groups", 1 if v else 1 << 30)  # forced on / off at any size
                option(b"split_max", v)
                for _ in range(3):
                    ctx.verify_batches_device(0, N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION, refs, stream)
                torch.cuda.synchronize()
                s0 = ctx.split_stats()
                ms = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    ctx.verify_batches_device(0, N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION, refs, stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                s1 = ctx.split_stats()
                print(f"K {K:3d} ({max(2, 128 // K):2d} leaders per group of 128) split_max {v:2d}: median {statistics.median(ms):.4f} ms "
                      f"min {min(ms):.4f} max {max(ms):.4f}; per launch {(s1['groups_split'] - s0['groups_split']) // args.reps} "
                      f"split groups, {(s1['high_points'] - s0['high_points']) // args.reps} high points", flush=True)
    finally:
        option(b"split_groups", 0)
        option(b"split_max", 0)
        ctx.close()


if __name__ == "__main__":
    main()
