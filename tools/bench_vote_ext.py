#!/usr/bin/env python3
"""Measurements behind the vote-extension path:

  kernel   k_vote_ext_signbytes alone (device events, tmv_kernel_timing) at
           payload sizes 0, 32, 256, 4 KiB, 64 KiB and 1 MiB and at a mix of one
           1 MiB payload among 32-byte ones, with the wave copy forced on
           (TMV_VOTE_EXT_WAVE_MIN=1) and off (=0), and a sweep of payload sizes
           16 .. 1024 for the cut-off
  commit   an extended commit of 150 and of 175 validators (2n signatures)
           through tmv_verify_extended_votes, its messages built on the host
           and on the device, alternating in one process with what the parent
           commit can do: two tmv_verify_batch_ex calls over host-built
           messages, votes then extensions
  window   a blocksync-sized window of 600 extended commits x 175, the same ways

The parent's way is timed over messages built before the clock starts (it has
no encoder for the extension messages; the figure is a lower bound of what a
caller of the parent would pay), the new entry point from C structs, message
building included.  Every figure is the median of --reps calls after one
warm-up, with min and max, wall clock around the synchronising call unless it
says device events.

  python tools/bench_vote_ext.py --out profiles/vote_ext/bench.json [--quick]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tendermint_amd import _native as N, host as H  # noqa: E402
from tendermint_amd.testing._openssl import Ed25519Signer  # noqa: E402
from tendermint_amd.types.canonical import (BlockID, PartSetHeader, Timestamp, vote_extension_sign_bytes,  # noqa: E402
                                            vote_sign_bytes)

CHAIN = "bench-chain"
KERNEL = "k_vote_ext_signbytes"
WAVE_KNOB, DEVICE_KNOB = "TMV_VOTE_EXT_WAVE_MIN", "TMV_VOTE_EXT_DEVICE_MIN"


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


# ---------------------------------------------------------------- kernel
def kernel_case(ctx, sizes, reps):
    """Device time of one k_vote_ext_signbytes launch over payloads of `sizes`,
    wave copy on and off, alternating."""
    rng = np.random.default_rng(1)
    off = np.zeros(len(sizes) + 1, np.uint32)
    off[1:] = np.cumsum(sizes)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    tmpl = np.zeros(len(sizes), np.uint32)
    tails = [H.vote_extension_template(CHAIN, 12345, 0)]
    out = {"entries": len(sizes), "payload_bytes": int(off[-1])}
    ts = {"wave": [], "lane": []}
    ref = None
    for rep in range(reps + 1):
        for way, knob in (("wave", "1"), ("lane", "0")):
            os.environ[WAVE_KNOB] = knob
            ctx.kernel_timing_read(KERNEL)
            msg, _ = ctx.vote_extension_sign_bytes_device(tails, tmpl, data, off)
            ms, cnt = ctx.kernel_timing_read(KERNEL)
            assert cnt == 1  # the wrapper's first call only sizes the messages
            if ref is None:
                ref = hashlib.sha256(msg).hexdigest()
            assert hashlib.sha256(msg).hexdigest() == ref, "wave and lane copies disagree"
            if rep:
                ts[way].append(ms / cnt)
    os.environ.pop(WAVE_KNOB, None)
    out["wave"], out["lane"] = stats(ts["wave"]), stats(ts["lane"])
    return out


def kernel_section(ctx, reps, quick):
    ctx.kernel_timing(True)
    res = {"timing": "device events around the launch (tmv_kernel_timing)", "sizes": {}, "sweep": {}}
    total = (4 if quick else 16) << 20
    for s in (0, 32, 256, 4096, 65536, 1 << 20):
        n = 100000 if s <= 256 else max(total // s, 1)
        res["sizes"][str(s)] = kernel_case(ctx, [s] * n, reps)
    mix = [32] * 4096
    mix[2000] = 1 << 20
    res["sizes"]["mix_1MiB_among_4095x32"] = kernel_case(ctx, mix, reps)
    for s in (16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024):
        res["sweep"][str(s)] = kernel_case(ctx, [s] * 100000, reps)
    # the cut-off: the smallest swept size from which the wave copy's median is never above the lane copy's
    cut = None
    for s in sorted(map(int, res["sweep"]), reverse=True):
        r = res["sweep"][str(s)]
        if r["wave"]["median_ms"] <= r["lane"]["median_ms"]:
            cut = s
        else:
            break
    res["cutoff_from_sweep"] = cut
    ctx.kernel_timing(False)
    return res


# ---------------------------------------------------------------- extended commits
class Window:
    """n_commits extended commits of n_vals validators, every precommit with a
    32..96-byte extension, as C structs for tmv_verify_extended_votes and as
    packed host-built batches for tmv_verify_batch_ex."""

    def __init__(self, n_commits, n_vals):
        signers = [Ed25519Signer(hashlib.sha256(b"bench val %d" % i).digest()) for i in range(n_vals)]
        addrs = [hashlib.sha256(s.public_key).digest()[:20] for s in signers]
        self.n = n_commits * n_vals
        self.keep = []
        self.arr = (H.CExtVoteIn * self.n)()
        vmsgs, emsgs, vsigs, esigs, pks = [], [], [], [], []
        k = H._Keep()
        for c in range(n_commits):
            bh = hashlib.sha256(b"block %d" % c).digest()
            bid = H.BlockID(bh, 3, bh)
            cb = H._c_block_id(k, bid)
            k.refs.append(cb)
            pbid = ctypes.pointer(cb)
            cbid = BlockID(bh, PartSetHeader(3, bh))
            for i, s in enumerate(signers):
                ts = (1700000000 + c, 1000 * i + 1)
                ext = hashlib.sha256(b"ext %d %d" % (c, i)).digest() * 3
                ext = ext[:32 + (c * 7 + i * 13) % 65]
                vm = vote_sign_bytes(CHAIN, 2, c + 1, 0, cbid, Timestamp(*ts))
                em = vote_extension_sign_bytes(CHAIN, c + 1, 0, ext)
                vs, es = s.sign(vm), s.sign(em)
                vmsgs.append(vm), emsgs.append(em), vsigs.append(vs), esigs.append(es), pks.append(s.public_key)
                a, al = k.buf(addrs[i])
                sg, sl = k.buf(vs)
                p, pl = k.buf(s.public_key)
                e, el = k.buf(ext)
                eg, egl = k.buf(es)
                self.arr[c * n_vals + i] = H.CExtVoteIn(
                    H.CVoteIn(2, c + 1, 0, pbid, ts[0], ts[1], a, al, sg, sl, N.TMV_KIND_ED25519, p, pl), e, el, eg, egl)
        self.keep.append(k)
        self.res = (ctypes.c_int32 * self.n)()
        self.failed = (ctypes.c_uint8 * self.n)()

        def pack(msgs, sigs):
            off = np.zeros(len(msgs) + 1, np.uint32)
            off[1:] = np.cumsum([len(m) for m in msgs])
            return (np.frombuffer(b"".join(pks), np.uint8).copy(), np.frombuffer(b"".join(sigs), np.uint8).copy(),
                    np.frombuffer(b"".join(msgs), np.uint8).copy(), off)
        self.votes_packed, self.exts_packed = pack(vmsgs, vsigs), pack(emsgs, esigs)


def commit_case(ctx, L, w, reps):
    def new_way(device_min):
        def f():
            os.environ[DEVICE_KNOB] = device_min
            rc = L.tmv_verify_extended_votes(ctx.handle, H.VOTE_MODE_VERIFY_AND_EXTENSION, CHAIN.encode(), w.arr, w.n,
                                             w.res, w.failed)
            assert rc == 0, rc
        return f

    def parent_way():
        for pk, sig, msg, off in (w.votes_packed, w.exts_packed):
            ok, _ = ctx.verify_batch_ex(N.TMV_KIND_ED25519, N.TMV_FLAG_KEY_CACHE, pk, sig, msg, off)
            assert ok

    ways = {"parent_two_batch_ex_calls_prebuilt_messages": parent_way,
            "extended_votes_host_built": new_way("4000000000"), "extended_votes_device_built": new_way("0")}
    ts = {k: [] for k in ways}
    for rep in range(reps + 1):
        for name, fn in ways.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ts[name].append(dt)
    os.environ.pop(DEVICE_KNOB, None)
    out = {"signatures": 2 * w.n}
    out.update({k: stats(v) for k, v in ts.items()})
    p = out["parent_two_batch_ex_calls_prebuilt_messages"]
    out["parent_spread_ms"] = round(p["max_ms"] - p["min_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vote_ext/bench.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a dry run of the tool)")
    ap.add_argument("--sections", default="kernel,commit,window")
    a = ap.parse_args()
    ctx = N.Context(1)
    L = H._setup_vote_ext(N.lib())
    res = {"tool": "tools/bench_vote_ext.py", "version": N.version(), "reps": a.reps, "quick": a.quick,
           "wave_min_default": N.VOTE_EXT_WAVE_MIN}
    sections = a.sections.split(",")
    if "kernel" in sections:
        res["kernel"] = kernel_section(ctx, a.reps, a.quick)
        print("kernel done", flush=True)
    if "commit" in sections:
        res["commit"] = {}
        for n_vals in (150, 175):
            res["commit"][str(n_vals)] = commit_case(ctx, L, Window(1, n_vals), a.reps)
        print("commit done", flush=True)
    if "window" in sections:
        n_commits = 60 if a.quick else 600
        res["window"] = {"commits": n_commits, "validators": 175}
        res["window"].update(commit_case(ctx, L, Window(n_commits, 175), a.reps))
        print("window done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
