#!/usr/bin/env python3
"""secp256k1 ECDSA verification rates on one GPU (tmv_secp256k1_verify_batch),
beside a host OpenSSL rate measured in the same run.

For 10,000 and 100,000 entries (honest commit-vote signatures plus 1% bad):
  kernel-only   k_secp_prep + k_secp_verify durations (tmv_kernel_timing)
  end-to-end    wall time of the host-buffer call: staging, H2D, both kernels,
                D2H (median of --reps calls after a warm-up)
and a 16-thread ECDSA_do_verify loop over the same signatures on the host's
CPUs, reported as {"kind": "proxy"}: libcrypto is not the reference's btcec
verifier, only a stand-in for a CPU's rate, as bench.py's cpu_baseline is.
The 100,000-entry batch repeats 10,000 distinct signatures ten times (the
kernels keep nothing between entries, so repetition does not change their
work).  Every run checks the verdicts against the batch's construction.

    python tools/bench_secp256k1.py [--out profiles/secp256k1/bench.json]

--cached measures tmv_secp256k1_verify_batch_ex with TMV_FLAG_KEY_CACHE (the
keys' comb tables kept on the device) against the uncached call instead: 150
entries of 150 keys, 175 keys x 600, and the two shapes above, the two calls
alternating in one session.  Per shape: the first cached call of a fresh
context (it builds every key's table), then medians with their spread of the
steady state (every key a hit) and of the uncached call, and the cached
kernels' durations.

    python tools/bench_secp256k1.py --cached [--out profiles/secp256k1_cache/bench.json]
"""
import argparse
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tendermint_amd import _native  # noqa: E402
from tendermint_amd.testing import secp256k1_factory as F  # noqa: E402


def tile(b: F.SecpBatch, times: int) -> F.SecpBatch:
    off = np.concatenate([[0]] + [b.off[1:].astype(np.uint64) + k * int(b.off[-1]) for k in range(times)])
    return F.SecpBatch(np.tile(b.pk, times), np.tile(b.sig, times), np.tile(b.msg, times), off.astype(np.uint32),
                       b.n * times, b.category * times)


def gpu_rates(ctx, b: F.SecpBatch, reps: int) -> dict:
    want = np.array([c == "honest" for c in b.category], np.uint8)
    ok, got = ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)  # warm-up: code objects, staging buffers
    assert np.array_equal(got, want) and not ok, "verdicts differ from the batch's construction"
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)  # synchronous: returns after the D2H copy
        wall.append(time.perf_counter() - t0)
    ctx.kernel_timing(True)
    try:
        for _ in range(reps):
            ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
        prep_ms, prep_n = ctx.kernel_timing_read("k_secp_prep")
        ver_ms, ver_n = ctx.kernel_timing_read("k_secp_verify")
    finally:
        ctx.kernel_timing(False)
    assert prep_n == ver_n and prep_n % reps == 0
    kernel_s = (prep_ms + ver_ms) / reps / 1e3
    med = float(np.median(wall))
    return {"n": b.n, "bad_entries": int((want == 0).sum()), "reps": reps,
            "k_secp_prep_ms": prep_ms / reps, "k_secp_verify_ms": ver_ms / reps,
            "kernel_only_verifies_per_s": b.n / kernel_s,
            "end_to_end_ms_median": med * 1e3, "end_to_end_ms_min": min(wall) * 1e3, "end_to_end_ms_max": max(wall) * 1e3,
            "end_to_end_verifies_per_s": b.n / med}


def spread(xs) -> dict:
    return {"median": float(np.median(xs)) * 1e3, "min": min(xs) * 1e3, "max": max(xs) * 1e3}


def cached_row(name: str, b: F.SecpBatch, reps: int) -> dict:
    """One shape, a context of its own: first cached call, then uncached and cached calls alternating."""
    want = np.array([c == "honest" for c in b.category], np.uint8)
    ctx = _native.Context(1)
    try:
        _, got = ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)  # warm-up: code objects, staging buffers
        assert np.array_equal(got, want), "verdicts differ from the batch's construction"
        t0 = time.perf_counter()
        _, got = ctx.secp256k1_verify_batch_ex(b.pk, b.sig, b.msg, b.off)
        first = time.perf_counter() - t0
        assert np.array_equal(got, want), "cached verdicts differ from the batch's construction"
        st0 = ctx.secp256k1_key_cache_stats()
        plain, cached = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
            plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, got = ctx.secp256k1_verify_batch_ex(b.pk, b.sig, b.msg, b.off)
            cached.append(time.perf_counter() - t0)
            assert np.array_equal(got, want)
        st1 = ctx.secp256k1_key_cache_stats()
        assert st1["misses"] == st0["misses"] and st1["hits"] > st0["hits"], "the steady state was not all hits"
        ctx.kernel_timing(True)
        try:
            for _ in range(reps):
                ctx.secp256k1_verify_batch_ex(b.pk, b.sig, b.msg, b.off)
                ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
            k = {n: ctx.kernel_timing_read(n) for n in ("k_secp_prep_cached", "k_secp_verify_comb", "k_secp_prep",
                                                        "k_secp_verify")}
        finally:
            ctx.kernel_timing(False)
        return {"shape": name, "n": b.n, "keys": st0["misses"], "reps": reps,
                "first_cached_call_ms": first * 1e3, "cached_steady_ms": spread(cached), "uncached_ms": spread(plain),
                "kernels_ms_per_call": {n: ms / reps for n, (ms, _) in k.items()},
                "key_table_bytes": st0["used"] * 61440}
    finally:
        ctx.close()


def cached_main(args):
    import torch
    fast = F.have_openssl()
    base = F.make_secp_batch(args.base_n, seed=0xBE7C, bad_frac=0.01, keys=175, fast=fast)
    shapes = [("150 entries x 150 keys", F.make_secp_batch(150, seed=0xC1, bad_frac=0.01, keys=150, fast=fast)),
              ("175 keys x 600", F.make_secp_batch(175 * 600, seed=0xC4, bad_frac=0.01, keys=175, fast=fast)),
              ("%d entries x 175 keys" % base.n, base), ("%d entries x 175 keys" % (10 * base.n), tile(base, 10))]
    res = {"device": torch.cuda.get_device_name(0), "version": _native.version(),
           "rows": [cached_row(name, b, args.reps) for name, b in shapes]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def openssl_rate(b: F.SecpBatch, threads: int, seconds: float) -> dict:
    """ECDSA_do_verify over the batch's honest entries on `threads` host threads
    (ctypes releases the interpreter lock during the call)."""
    if not F.have_openssl():
        return {"kind": "proxy", "error": "libcrypto with secp256k1 not found"}
    L = F._openssl()
    honest = [i for i in range(b.n) if b.category[i] == "honest"][:2048]
    counts = [0] * threads
    stop = time.perf_counter() + seconds

    def work(t):
        items = []
        keys = {}
        for i in honest[t::threads]:
            pk, msg, sig = b.entry(i)
            key = keys.setdefault(pk, F.OpensslKey(pk))
            s = L.ECDSA_SIG_new()
            L.ECDSA_SIG_set0(s, L.BN_bin2bn(sig[:32], 32, None), L.BN_bin2bn(sig[32:], 32, None))
            items.append((hashlib.sha256(msg).digest(), s, key.key))
        n = 0
        while time.perf_counter() < stop:
            for z, s, k in items:
                if L.ECDSA_do_verify(z, 32, s, k) != 1:
                    raise RuntimeError("OpenSSL rejects an honest signature")
            n += len(items)
        counts[t] = n

    t0 = time.perf_counter()
    ths = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    dt = time.perf_counter() - t0
    return {"kind": "proxy", "what": "OpenSSL ECDSA_do_verify (secp256k1), SHA-256 digests precomputed",
            "threads": threads, "seconds": dt, "verifies": sum(counts), "verifies_per_s": sum(counts) / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cached", action="store_true", help="cached vs uncached rows (see the module text)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-seconds", type=float, default=4.0)
    ap.add_argument("--base-n", type=int, default=10000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_secp256k1.py needs a GPU (there is no CPU fallback)")
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "secp256k1_cache" if args.cached else "secp256k1", "bench.json")
    if args.cached:
        return cached_main(args)
    t0 = time.perf_counter()
    base = F.make_secp_batch(args.base_n, seed=0xBE7C, bad_frac=0.01, keys=175, fast=F.have_openssl())
    gen_s = time.perf_counter() - t0
    ctx = _native.Context(1)
    res = {"device": torch.cuda.get_device_name(0), "version": _native.version(), "input_generation_s": gen_s,
           "gpu": [gpu_rates(ctx, base, args.reps), gpu_rates(ctx, tile(base, 10), args.reps)],
           "cpu_openssl": openssl_rate(base, args.threads, args.cpu_seconds)}
    ctx.close()
    cpu = res["cpu_openssl"].get("verifies_per_s")
    if cpu:
        g = res["gpu"][1]
        res["faster"] = "gpu" if g["end_to_end_verifies_per_s"] > cpu else "cpu_openssl_proxy"
        res["gpu_end_to_end_over_cpu_proxy_at_100k"] = g["end_to_end_verifies_per_s"] / cpu
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
