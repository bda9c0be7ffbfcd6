#!/usr/bin/env python3
"""Bucket entries per signature of the benchmark's launch (256 C2 batches
cycling through 64 resident ones) from tmv_bucket_entry_stats, at the default
column tile (64), in batch order (0) and at tiles 32 and 128:

  python tools/entries_per_sig.py
Prints one JSON line per tile (profiles/key_runs/entries.txt)."""
import ctypes
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tendermint_amd.testing.factory import make_c2_batch, C2_VALID_KINDS
from tendermint_amd import _native as N
import torch

def _c2(seed):
    return make_c2_batch(10_000, seed=seed)

def main():
    with ProcessPoolExecutor(16) as ex:
        base = list(ex.map(_c2, [0xED25519 + j for j in range(64)]))
    dev = torch.device("cuda:0")
    L = N.lib()
    L.tmv_internal_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    ctx = N.Context(1)
    ctx.set_batch_options(stats=True)
    res = []
    for b in base:
        t = {f: torch.from_numpy(getattr(b, f)).to(dev) for f in ("pk", "sig", "msg")}
        t["off"] = torch.from_numpy(b.off.view(np.int32)).to(dev)
        res.append(t)
    outs = [torch.zeros(10_000, dtype=torch.int8, device=dev) for _ in range(256)]
    refs = [N.BatchRef(res[j % 64]["pk"].data_ptr(), res[j % 64]["sig"].data_ptr(), res[j % 64]["msg"].data_ptr(),
                       res[j % 64]["off"].data_ptr(), 10_000, int(base[j % 64].off[-1]), outs[j].data_ptr())
            for j in range(256)]
    for tile in (-1, 0, 32, 128):
        assert L.tmv_internal_option(b"column_tile", tile) == 0
        torch.cuda.synchronize()
        e0 = ctx.bucket_entry_stats()
        ctx.verify_batches_device(0, N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION, refs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        e1 = ctx.bucket_entry_stats()
        ok = all(np.array_equal(outs[j].cpu().numpy(), np.array([k in C2_VALID_KINDS for k in base[j % 64].kinds], np.int8))
                 for j in (0, 63, 64, 255))
        print(json.dumps({"column_tile": tile, "entries_per_signature": round((e1 - e0) / 2.56e6, 3), "exact": ok}), flush=True)
    ctx.close()

if __name__ == "__main__":
    main()
