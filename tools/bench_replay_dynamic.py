#!/usr/bin/env python3
"""Measurements behind blocksync_replay_dynamic:

  schedule  the host cost of the validator schedule alone, no engine
              cpp     tmv_validator_set_update + tmv_validator_set_rotate chained over C arrays, one thread:
                      the arithmetic itself
              python  chains._Schedule over the same records: what the driver pays (the arithmetic, the
                      conversion of every new set to Python objects and back, the params)
            at config 4's shape (175 validators, 10,000 blocks, a change every 100 blocks) and at 10,000
            validators x 600 blocks with a change every block
  static    a 600-block, 175-validator chain without updates on the engine: blocksync_replay_dynamic and
            blocksync_replay_stateful (of this revision, or of --parent-chains FILE) alternating in one process

Every figure is the median of --reps runs (default 15) after one warm-up, with min and max.

  python tools/bench_replay_dynamic.py --out profiles/valset_updates/bench.json [--quick] [--no-engine]
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
from tendermint_amd import _native, chains, host as H  # noqa: E402


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "reps": len(xs)}


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def key(i: int) -> bytes:
    return hashlib.sha256(b"bench key %d" % i).digest()


def records_for(n_vals: int, n_blocks: int, every: int):
    """(genesis set, records): every `every` blocks one validator's power changes, one leaves and one joins."""
    vals = H.new_validator_set([(0, key(i), 10 + i % 7) for i in range(n_vals)])
    records, nxt = [], n_vals
    members = list(range(n_vals))
    for g in range(n_blocks):
        ups = []
        if g % every == every - 1:
            out = members.pop((7 * g) % len(members))
            members.append(nxt)
            ups = [(0, key(members[(3 * g) % (len(members) - 1)]), 5 + g % 11), (0, key(out), 0), (0, key(nxt), 9)]
            nxt += 1
        records.append(chains.BlockRecord([], b"", ups))
    return vals, records


def schedule_cpp(L, vals: H.ValidatorSet, records):
    """The update and rotate calls of the schedule over C arrays alone: the
    output array of one call is the input of the next."""
    vp, up = ctypes.POINTER(H.CValidator), ctypes.POINTER(H.CValidatorUpdate)
    k = H._Keep()
    H._c_validators(k, vals)
    cur = k.refs[-1].copy()
    n = len(vals.validators)
    dt = cur.dtype
    prepared = []
    for r in records:
        if r.validator_updates:
            u, nu, _ = H._c_updates(k, r.validator_updates)
            prepared.append((u, nu, (ctypes.c_uint8 * (20 * nu))()))
        else:
            prepared.append(None)
    err = ctypes.create_string_buffer(512)
    props = (ctypes.c_int32 * len(records))()
    n_out = ctypes.c_uint32(0)
    keep = [cur, k]  # k owns the key bytes that every array points into

    def run():
        nonlocal cur, n
        cur, n, pending = keep[0].copy(), len(vals.validators), 0
        for pr in prepared:
            if pr is not None:
                if pending:
                    assert L.tmv_validator_set_rotate(ctypes.cast(cur.ctypes.data, vp), n, 1, pending, props, err, 512) == 0
                    pending = 0
                u, nu, scratch = pr
                out = np.zeros(n + nu, dtype=dt)
                rc = L.tmv_validator_set_update(ctypes.cast(cur.ctypes.data, vp), n, ctypes.cast(u.ctypes.data, up), nu, 1,
                                                ctypes.cast(scratch, H._u8p), ctypes.cast(out.ctypes.data, vp), n + nu,
                                                ctypes.byref(n_out), err, 512)
                assert rc == 0, err.value
                cur, n = out, n_out.value
            pending += 1
        if pending:
            assert L.tmv_validator_set_rotate(ctypes.cast(cur.ctypes.data, vp), n, 1, pending, props, err, 512) == 0
    return run


def bench_schedule(reps: int, quick: bool):
    L = H._setup_valset(_native.lib())
    out = {}
    shapes = {"c4_175x10000_every100": (175, 10000, 100), "10000x600_every1": (10000, 600, 1)}
    if quick:
        shapes = {"quick_50x200_every10": (50, 200, 10), "quick_500x20_every1": (500, 20, 1)}
    for name, (n_vals, n_blocks, every) in shapes.items():
        vals, records = records_for(n_vals, n_blocks, every)
        state = chains.ReplayState(chain_id="bench", validators=vals, app_hash=b"", last_results_hash=b"")
        sc = chains._Schedule(state, records, n_blocks, None)
        assert sc.failed is None and len(sc.sets) == n_blocks + 3
        out[name] = {"validators": n_vals, "blocks": n_blocks, "change_every": every,
                     "changes": sum(1 for r in records if r.validator_updates),
                     "cpp": stats(wall(schedule_cpp(L, vals, records), reps)),
                     "python": stats(wall(lambda: chains._Schedule(state, records, n_blocks, None), reps))}
        print(name, json.dumps(out[name]), flush=True)
    return out


def load_parent(path: str):
    """Another revision's tendermint_amd/chains.py, loaded beside this one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tendermint_amd.chains_parent", path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m
    spec.loader.exec_module(m)
    return m


def bench_static(reps: int, quick: bool, parent: str = None):
    from tendermint_amd.testing.blocks import make_stateful_chain
    old = load_parent(parent) if parent else chains
    n_blocks, n_vals = (60, 20) if quick else (600, 175)
    ctx = _native.Context(1)
    state, blocks, _, records = make_stateful_chain(n_blocks + 1, n_vals, seed=5, raw_len=(200, 2000), part_size=65536)
    want = (n_blocks, None)
    stateful = lambda: old.blocksync_replay_stateful(ctx, state, blocks, records)  # noqa: E731
    dynamic = lambda: chains.blocksync_replay_dynamic(ctx, state, blocks, records)[:2]  # noqa: E731
    assert stateful() == want and dynamic() == want
    ts = {"stateful": [], "dynamic": []}
    for _ in range(reps):
        for name, fn in (("stateful", stateful), ("dynamic", dynamic)):
            t0 = time.perf_counter()
            assert fn() == want
            ts[name].append((time.perf_counter() - t0) * 1e3)
    out = {"blocks": n_blocks, "validators": n_vals, "stateful_from": parent or "this revision", "stateful": stats(ts["stateful"]), "dynamic": stats(ts["dynamic"])}
    out["dynamic_median_inside_stateful_range"] = (out["stateful"]["min_ms"] <= out["dynamic"]["median_ms"]
                                                   <= out["stateful"]["max_ms"])
    ctx.close()
    print("static", json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-engine", action="store_true", help="the schedule alone (no GPU needed)")
    ap.add_argument("--parent-chains", help="a chains.py of another revision: its blocksync_replay_stateful is the baseline")
    a = ap.parse_args()
    doc = {"schedule": bench_schedule(a.reps, a.quick)}
    if not a.no_engine:
        doc["static"] = bench_static(a.reps, a.quick, a.parent_chains)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
