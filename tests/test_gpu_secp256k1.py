"""secp256k1 ECDSA verification on the device (tmv_secp256k1_verify_batch /
tmv_secp256k1_verify, secp256k1_kernels.hip) and secp256k1 validators through
the host layer of libtmgpu.so.  Expected verdicts are the big-integer
restatement's (tests/secp256k1_ref.py), cross-checked with OpenSSL when the
golden files were written (tests/golden/make_secp256k1_golden.py)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import commit_fixtures as CF
import secp256k1_cases as SC
import secp256k1_ref as R
from tendermint_amd import _native, host as H
from tendermint_amd.testing import secp256k1_factory as F
from tendermint_amd.testing.factory import make_c2_batch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pack(entries):
    """[(pk33, msg, sig64)] -> packed arrays."""
    off = np.zeros(len(entries) + 1, np.uint32)
    off[1:] = np.cumsum([len(m) for _, m, _ in entries])
    cat = lambda k: np.frombuffer(b"".join(e[k] for e in entries), np.uint8).copy()  # noqa: E731
    return cat(0), cat(2), cat(1), off


@pytest.fixture(scope="module")
def vectors(golden):
    return golden("secp256k1_vectors.json")


@pytest.fixture(scope="module")
def big():
    """The generated 4,096-entry batch and the restatement's stored verdicts."""
    with open(os.path.join(GOLDEN, "secp256k1_batch4096.json")) as f:
        g = json.load(f)
    b = F.make_secp_batch(g["n"], seed=g["seed"])
    assert F.batch_digest(b) == g["sha256"], "the generated batch is not the one the stored verdicts belong to"
    bits = bytes.fromhex(g["valid_bits"])
    want = np.array([(bits[i >> 3] >> (i & 7)) & 1 for i in range(b.n)], np.uint8)
    # the stored verdicts against the restatement, run here: every corrupted entry and a sample of honest ones
    for i in [i for i in range(b.n) if b.category[i] != "honest"] + list(range(0, b.n, 128)):
        assert R.verify(*b.entry(i)) == bool(want[i]), (i, b.category[i])
    return b, want


def test_golden_vectors_one_call(ctx, vectors):
    ent = [(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in vectors]
    pk, sig, msg, off = pack(ent)
    ok, got = ctx.secp256k1_verify_batch(pk, sig, msg, off)
    want = np.array([int(v["valid"]) for v in vectors], np.uint8)
    bad = [vectors[i]["name"] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    assert not ok


def test_golden_vectors_one_by_one(ctx, vectors):
    for v in vectors:
        pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        assert ctx.secp256k1_verify(pk, msg, sig) == v["valid"], v["name"]
    v = vectors[0]
    pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
    assert v["valid"]
    for bad_pk in (pk[:32], pk + b"\0", b"\x04" + pk[1:] + bytes(32), b""):
        assert ctx.secp256k1_verify(bad_pk, msg, sig) is False
    for bad_sig in (sig[:63], sig + b"\0", b""):
        assert ctx.secp256k1_verify(pk, msg, bad_sig) is False


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4096])
def test_batches_bit_exact(ctx, big, n):
    b, want = big
    p = b.prefix(n)
    ok, got = ctx.secp256k1_verify_batch(p.pk, p.sig, p.msg, p.off)
    assert np.array_equal(got, want[:n]), [(i, p.category[i]) for i in np.nonzero(got != want[:n])[0]]
    assert ok == bool(want[:n].all())
    if n == 4096:
        assert 0.03 < 1 - want.mean() < 0.08 and len(set(b.category)) == 1 + len(F.CORRUPTIONS)


def test_all_valid_batch_and_parse_failures_in_lanes_0_and_63(ctx):
    honest = F.make_secp_batch(130, seed=9, bad_frac=0.0)
    ok, got = ctx.secp256k1_verify_batch(honest.pk, honest.sig, honest.msg, honest.off)
    assert ok and got.all()
    bad_at = (0, 63, 64, 127)  # first and last lane of the first two waves
    b = F.make_secp_batch(130, seed=9, bad_frac=0.0, bad_at=bad_at)
    assert all(R.parse_pubkey(b.entry(i)[0]) is None for i in bad_at)
    ok, got = ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
    assert not ok
    assert list(np.nonzero(got == 0)[0]) == list(bad_at)  # the neighbours are undisturbed


def test_every_message_length_0_to_130(ctx):
    lens = list(range(131))
    b = F.make_secp_batch(len(lens), seed=3, bad_frac=0.0, keys=4, msg_lens=lens)
    assert [int(b.off[i + 1] - b.off[i]) for i in range(b.n)] == lens
    ok, got = ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
    assert ok and got.all()
    for i in range(0, b.n, 10):
        assert R.verify(*b.entry(i))
    # the same batch with every message's last byte changed (length 0: the signature instead)
    msg = b.msg.copy()
    msg[b.off[1:][1:] - 1] ^= 0x80
    sig = b.sig.copy()
    sig[5] ^= 1
    ok, got = ctx.secp256k1_verify_batch(b.pk, sig, msg, b.off)
    assert not ok and not got.any()


def test_commit_cases_150_validators(ctx):
    SC.check_commit_cases(CF.GpuBackend(ctx), 150, "ed25519")


def test_light_window_of_8_headers(ctx):
    jobs, vals = SC.light_window(8, 12)
    assert H.light_verify_many(ctx, jobs) == [(H.LIGHT_OK, None)] * 8
    # a bad signature in the sixth header's commit fails that job alone
    jb = jobs[5]
    bad = SC.flip(jb.untrusted.commit.signatures[0].signature)
    jobs[5] = H.LightJob(jb.trusted, jb.trusted_next_vals,
                         H.SignedHeader(jb.untrusted.header, SC.with_sig(jb.untrusted.commit, 0, bad)),
                         jb.untrusted_vals, jb.trusting_period_ns, jb.now)
    res = H.light_verify_many(ctx, jobs)
    assert [c for c, _ in res] == [H.LIGHT_OK] * 5 + [H.LIGHT_ERR_INVALID_HEADER] + [H.LIGHT_OK] * 2
    assert "wrong signature (#0): " + bad.hex().upper() in res[5][1]


def test_argument_errors_and_metrics(ctx):
    L = _native.lib()
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))  # noqa: E731
    b = F.make_secp_batch(5, seed=1, bad_frac=0.0)
    out = np.zeros(8, np.uint8)
    call = lambda pk, sig, msg, off, n, o: L.tmv_secp256k1_verify_batch(ctx.handle, pk, sig, msg, off, n, o)  # noqa: E731
    good = (u8(b.pk), u8(b.sig), u8(b.msg), u32(b.off), 5, u8(out))
    assert call(*good) == _native.TMV_ALL_VALID
    assert call(*good[:4], 0, good[5]) == _native.TMV_NOT_ALL  # an empty batch verifies false
    for k in (0, 1, 3, 5):  # null pk, sig, msg_off, valid_out
        args = list(good)
        args[k] = None
        assert call(*args) == -1, k
    args = list(good)
    args[2] = None  # null msg with message bytes
    assert call(*args) == -1
    off = b.off.copy()
    off[0] = 1
    assert call(good[0], good[1], good[2], u32(off), 5, good[5]) == -1
    off = b.off.copy()
    off[3] = off[2] - 1
    assert call(good[0], good[1], good[2], u32(off), 5, good[5]) == -1
    assert call(*good[:4], (1 << 26) + 1, good[5]) == -1
    off = np.array([0, (1 << 30) + 1], np.uint32)
    assert call(good[0], good[1], good[2], u32(off), 1, good[5]) == -1
    assert "tmv_secp256k1_verify_batch" in _native.last_error()
    # the context still verifies, and counts the calls and entries
    c2 = make_c2_batch(300, seed=5)
    ok, got = ctx.ed25519_verify_batch(c2.pk, c2.sig, c2.msg, c2.off)
    assert got.sum() > 250
    m0 = ctx.metrics()
    assert call(*good) == _native.TMV_ALL_VALID
    assert ctx.secp256k1_verify(*b.entry(0))
    m1 = ctx.metrics()
    assert m1["calls"] - m0["calls"] == 2 and m1["signatures"] - m0["signatures"] == 6
    assert m1["max_batch"] >= 5


def test_kernel_timing_names(ctx):
    b = F.make_secp_batch(64, seed=2, bad_frac=0.0)
    ctx.kernel_timing(True)
    try:
        ctx.secp256k1_verify_batch(b.pk, b.sig, b.msg, b.off)
        for name in ("k_secp_prep", "k_secp_verify"):
            ms, launches = ctx.kernel_timing_read(name)
            assert launches == 1 and ms > 0
    finally:
        ctx.kernel_timing(False)
