"""secp256k1 verification against keys cached on the device as comb tables
(tmv_secp256k1_verify_batch_ex with TMV_FLAG_KEY_CACHE: k_secp_key_table,
k_secp_prep_cached, k_secp_verify_comb, and the runtime's LRU of key slots).
Expected verdicts are the big-integer restatement's (tests/secp256k1_ref.py)
or the golden file's; the uncached call must agree entry by entry."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import commit_fixtures as CF
import secp256k1_cases as SC
import secp256k1_comb_cases as CC
import secp256k1_ref as R
from tendermint_amd import _native, host as H
from tendermint_amd.testing import secp256k1_factory as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = R.N, R.P
TIMED = ("k_secp_key_table", "k_secp_prep_cached", "k_secp_verify_comb", "k_secp_prep", "k_secp_verify")


def pack(entries):
    """[(pk33, msg, sig64)] -> packed arrays."""
    off = np.zeros(len(entries) + 1, np.uint32)
    off[1:] = np.cumsum([len(m) for _, m, _ in entries])
    cat = lambda k: np.frombuffer(b"".join(e[k] for e in entries), np.uint8).copy()  # noqa: E731
    return cat(0), cat(2), cat(1), off


def both(ctx, entries):
    """Verdicts of the cached and the uncached call, which must be equal."""
    a = pack(entries)
    _, cached = ctx.secp256k1_verify_batch_ex(*a)
    _, plain = ctx.secp256k1_verify_batch(*a)
    assert np.array_equal(cached, plain), list(np.nonzero(cached != plain)[0])
    return [bool(v) for v in cached]


def ref_verdicts(entries):
    combs = {}
    for pk, _, _ in entries:
        q = R.parse_pubkey(pk)
        if q is not None and pk not in combs:
            combs[pk] = R.comb_table(q)
    return [R.verify(pk, msg, sig, combs) for pk, msg, sig in entries]


@pytest.fixture(scope="module")
def signers():
    return [F.Secp256k1Signer.from_secret(b"cache key: %d" % i) for i in range(3)]


@pytest.fixture(scope="module")
def vectors(golden):
    vs = golden("secp256k1_vectors.json")
    return vs, [(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in vs]


def test_golden_vectors_cached_uncached_and_stats(ctx, vectors):
    """`ctx` only orders this test after the session's context: the contexts
    opened here come second, as everywhere else in the suite."""
    vs, ent = vectors
    want = np.array([int(v["valid"]) for v in vs], np.uint8)
    parsable = {pk for pk, _, _ in ent if R.parse_pubkey(pk) is not None}
    assert 0 < len(parsable) < len({pk for pk, _, _ in ent})
    own = _native.Context(1)  # its own context: the counters start at zero
    try:
        a = pack(ent)
        _, plain = own.secp256k1_verify_batch(*a)
        assert own.secp256k1_key_cache_stats()["used"] == 0
        ok, got = own.secp256k1_verify_batch_ex(*a)
        bad = [vs[i]["name"] for i in np.nonzero(got != want)[0]]
        assert not bad and not ok, bad
        assert np.array_equal(got, plain)
        s1 = own.secp256k1_key_cache_stats()
        assert (s1["misses"], s1["hits"], s1["used"]) == (len(parsable), 0, len(parsable)), s1
        _, again = own.secp256k1_verify_batch_ex(*a)
        assert np.array_equal(again, want)
        s2 = own.secp256k1_key_cache_stats()
        assert (s2["misses"], s2["hits"], s2["used"]) == (len(parsable), len(parsable), len(parsable)), s2
        # flags: 0 is the uncached call, any other bit an argument error
        _, zero = own.secp256k1_verify_batch_ex(*a, flags=0)
        assert np.array_equal(zero, want) and own.secp256k1_key_cache_stats() == s2
        with pytest.raises(_native.NativeError):
            own.secp256k1_verify_batch_ex(*a, flags=2)
    finally:
        own.close()


def test_one_entry_and_257_over_three_keys(ctx, signers):
    one = [(signers[0].public_key, b"one", signers[0].sign(b"one"))]
    assert both(ctx, one) == ref_verdicts(one) == [True]
    rng = random.Random(257)
    ent = []
    for i in range(257):  # two blocks and one tail lane; a wave holds all three keys
        s = signers[i % 3]
        msg = b"vote %d" % i
        sig = s.sign(msg)
        if i in (0, 63, 64, 255, 256) or rng.random() < 0.05:
            sig = SC.flip(sig)
        ent.append((s.public_key, msg, sig))
    want = ref_verdicts(ent)
    assert want.count(False) >= 5 and not want[256]
    assert both(ctx, ent) == want
    assert both(ctx, ent) == want  # every key a hit


def test_bad_keys_beside_good_ones(ctx, signers):
    s = signers[0]
    rng = random.Random(4)
    x = s.public_key[1:]
    bad_keys = [b"\x00" + x, b"\x04" + x, b"\x02" + P.to_bytes(32, "big"),
                b"\x02" + F.non_residue_x(rng).to_bytes(32, "big")]
    assert all(R.parse_pubkey(k) is None for k in bad_keys)
    ent = []
    for i, k in enumerate(bad_keys):
        for key in (s.public_key, k, signers[1].public_key):
            msg = b"beside %d" % len(ent)
            signer = s if key != signers[1].public_key else signers[1]
            ent.append((key, msg, signer.sign(msg)))
    both(ctx, [e for e in ent if e[0] not in bad_keys])  # the good keys are in the cache now
    used = ctx.secp256k1_key_cache_stats()["used"]
    for _ in range(2):
        got = both(ctx, ent)
        assert got == [e[0] not in bad_keys for e in ent] == ref_verdicts(ent)
        assert ctx.secp256k1_key_cache_stats()["used"] == used
    ctx.kernel_timing(True)  # a key without a square root is remembered, not built again
    try:
        assert both(ctx, ent) == ref_verdicts(ent)
        assert ctx.kernel_timing_read("k_secp_key_table")[1] == 0
    finally:
        for name in TIMED:  # leave no recorded launch behind for other tests' counts
            ctx.kernel_timing_read(name)
        ctx.kernel_timing(False)
    only_bad = [e for e in ent if e[0] in bad_keys]
    assert both(ctx, only_bad) == [False] * 4
    assert ctx.secp256k1_key_cache_stats()["used"] == used


def test_bad_signatures_under_the_cached_path(ctx, signers):
    s = signers[2]
    msg = b"a message to corrupt"
    sig = s.sign(msg)
    r, sv = sig[:32], sig[32:]
    b32 = lambda v: v.to_bytes(32, "big")  # noqa: E731
    bit = lambda b, i: b[:i] + bytes([b[i] ^ 0x10]) + b[i + 1:]  # noqa: E731
    ent = [(s.public_key, msg, sig),
           (s.public_key, msg, b32(0) + sv), (s.public_key, msg, r + b32(0)),
           (s.public_key, msg, b32(N) + sv), (s.public_key, msg, r + b32(N)),
           (s.public_key, msg, r + b32(N - int.from_bytes(sv, "big"))),
           (s.public_key, msg, bit(r, 7) + sv), (s.public_key, msg, r + bit(sv, 20)),
           (s.public_key, bit(msg, 3), sig), (bit(s.public_key, 9), msg, sig)]
    want = ref_verdicts(ent)
    assert want == [True] + [False] * 9
    assert both(ctx, ent) == want


def test_key_one_signatures_doubling_case(ctx):
    cases = CC.key1_cases()
    assert [c for _, _, c in cases] == [True] * 4 + [False] * 4
    pk = R.compress(R.G)
    ent = [(pk, msg, sig) for msg, sig, _ in cases]
    ent += [(pk, msg, sig[:40] + bytes([sig[40] ^ 4]) + sig[41:]) for msg, sig, _ in cases]
    want = ref_verdicts(ent)
    assert want == [True] * 8 + [False] * 8
    assert both(ctx, ent) == want


def _child(code, **env):
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_eviction_capacity_two():
    """Capacity 2: three keys over three calls of two keys each evict (more
    misses than distinct keys); one call with three distinct keys takes the
    uncached path.  Verdicts against the restatement throughout."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import secp256k1_ref as R
import test_gpu_secp256k1_cache as T
from tendermint_amd import _native
from tendermint_amd.testing import secp256k1_factory as F
ctx = _native.Context(1)
keys = [F.Secp256k1Signer.from_secret(b"evict: %d" % i) for i in range(3)]
def entries(which, tag):
    ent = []
    for t in range(6):
        s = keys[which[t % len(which)]]
        msg = b"%s %d" % (tag, t)
        sig = s.sign(msg)
        ent.append((s.public_key, msg, sig if t != 4 else bytes([sig[0] ^ 1]) + sig[1:]))
    return ent
for rnd, which in enumerate(((0, 1), (1, 2), (2, 0))):
    ent = entries(which, b"round %d" % rnd)
    want = T.ref_verdicts(ent)
    assert want.count(False) == 1
    assert T.both(ctx, ent) == want, rnd
s = ctx.secp256k1_key_cache_stats()
assert s["capacity"] == 2 and s["used"] == 2 and s["misses"] == 4 and s["hits"] == 2, s
ent = entries((0, 1, 2), b"three")
assert T.both(ctx, ent) == T.ref_verdicts(ent)
assert ctx.secp256k1_key_cache_stats() == s  # the uncached path: the cache is untouched
ent = entries((2, 0), b"after")
assert T.both(ctx, ent) == T.ref_verdicts(ent)
s2 = ctx.secp256k1_key_cache_stats()
assert s2["misses"] == 4 and s2["hits"] == 4, s2
print("ok", s2)
"""
    assert "ok" in _child(code, TMV_SECP_KEY_CACHE_CAPACITY="2")


def test_commits_through_the_host_layer_match_the_uncached_engine(ctx):
    """8 commits of 7 secp256k1 validators through tmv_verify_commits, twice:
    results and error texts equal those of a process whose cache is off."""
    code = r"""
import sys, json
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import secp256k1_comb_cases as CC
from tendermint_amd import _native, host as H
ctx = _native.Context(1)
jobs = CC.commit_jobs()
res = [H.verify_commits(ctx, jobs), H.verify_commits(ctx, jobs)]
s = ctx.secp256k1_key_cache_stats()
assert s["capacity"] == 0 and s["used"] == 0 and s["misses"] == 0, s
print("RESULT " + json.dumps(res))
"""
    out = _child(code, TMV_SECP_KEY_CACHE_CAPACITY="0")
    want = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
    jobs = CC.commit_jobs()
    bad = jobs[5].commit.signatures[3].signature
    assert want[0] == want[1] == [None] * 5 + ["wrong signature (#3): " + bad.hex().upper()] + [None] * 2
    s0 = ctx.secp256k1_key_cache_stats()
    assert s0["capacity"] >= 7
    for rnd in range(2):
        assert H.verify_commits(ctx, jobs) == want[rnd]
    s1 = ctx.secp256k1_key_cache_stats()
    assert s1["hits"] + s1["misses"] - s0["hits"] - s0["misses"] == 14  # 7 keys per call: the cached call ran


def test_mixed_set_cases_keep_their_texts(ctx):
    SC.check_commit_cases(CF.GpuBackend(ctx), 7, "ed25519")


def test_two_logical_devices(ctx, vectors):
    vs, ent = vectors
    want = np.array([int(v["valid"]) for v in vs], np.uint8)
    two = _native.Context(1, logical=2)
    try:
        assert two.num_devices() == 2
        a = pack(ent)
        for _ in range(2):
            _, got = two.secp256k1_verify_batch_ex(*a)
            assert np.array_equal(got, want)
        _, plain = two.secp256k1_verify_batch(*a)
        assert np.array_equal(plain, want)
    finally:
        two.close()


def test_kernel_timing_names(ctx, signers):
    ent = [(signers[0].public_key, b"timed", signers[0].sign(b"timed")),
           (F.Secp256k1Signer.from_secret(b"timed key").public_key, b"timed", signers[0].sign(b"timed"))]
    a = pack(ent)
    ctx.kernel_timing(True)
    try:
        for name in TIMED:  # forget what earlier timed runs recorded
            ctx.kernel_timing_read(name)
        ctx.secp256k1_verify_batch_ex(*a)
        for name in ("k_secp_prep_cached", "k_secp_verify_comb"):
            ms, launches = ctx.kernel_timing_read(name)
            assert launches == 1 and ms > 0, name
        ms, launches = ctx.kernel_timing_read("k_secp_key_table")
        assert launches == 1 and ms > 0  # no other test uses the second key
    finally:
        ctx.kernel_timing(False)
