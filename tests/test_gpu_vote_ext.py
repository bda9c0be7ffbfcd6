"""Vote-extension sign-bytes on the device (k_vote_ext_signbytes,
tmv_verify_votes_and_extensions): the messages the device writes equal the
checker's (vote_ext_ref.py) byte for byte, and verification over vote and
extension entries in one batch gives the oracle's statuses."""
import random

import numpy as np
import pytest

import oracle_c as C
import vote_cases as V
import vote_ext_cases as X
import vote_ext_ref as R
from tendermint_amd import _native as N
from tendermint_amd.testing._openssl import Ed25519Signer
from tendermint_amd.testing.factory import Batch, key_seed

pytestmark = pytest.mark.gpu


def _check_bytes(ctx, e: X.Entries):
    got, off = ctx.vote_extension_sign_bytes_device(e.tails, e.tmpl, e.data, e.off)
    want, want_off = e.expected()
    assert np.array_equal(off, want_off)
    if got != want:  # name the first entry that differs, not a megabyte of bytes
        for i in range(len(e.entries)):
            a, b = int(want_off[i]), int(want_off[i + 1])
            assert got[a:b] == want[a:b], "entry %d (payload of %d bytes)" % (i, len(e.entries[i][1]))
    assert got == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_bytes_entry_counts(ctx, n):
    _check_bytes(ctx, X.random_entries(random.Random(700 + n), 7, n))


def test_bytes_lengths_at_every_source_offset(ctx):
    _check_bytes(ctx, X.length_offset_entries(random.Random(71)))


def test_bytes_varint_boundaries(ctx):
    rng = random.Random(72)
    want = [R.ext_len_for_body(*X.BOUNDARY_TEMPLATE, b) for b in (127, 128, 16383, 16384)]
    assert want == X.BOUNDARY_LENGTHS
    e = X.Entries([X.BOUNDARY_TEMPLATE], [(0, X.payload(rng, ln)) for ln in X.BOUNDARY_LENGTHS])
    assert [len(m) for m in e.msgs] == [128, 130, 16385, 16387]
    _check_bytes(ctx, e)


def test_bytes_every_tail_combination(ctx):
    rng = random.Random(73)
    ents = [(t, X.payload(rng, ln)) for t in range(len(X.TAIL_COMBOS)) for ln in (0, 5, 200)]
    _check_bytes(ctx, X.Entries(X.TAIL_COMBOS, ents))


def test_bytes_one_byte_messages_beside_long_ones(ctx):
    """300 all-empty entries (the message is the single byte 00) with a
    64 KiB entry at each end and in the middle: a store that leaves its entry
    lands in a neighbour's only byte."""
    rng = random.Random(74)
    big = lambda: (0, X.payload(rng, 65536))
    ents = [big()] + [(0, b"")] * 150 + [big()] + [(0, b"")] * 150 + [big()]
    e = X.Entries([("", 0, 0)], ents)
    assert e.msgs[1] == b"\x00"
    _check_bytes(ctx, e)


def test_bytes_one_mib_in_a_wave_of_empty_entries(ctx):
    rng = random.Random(75)
    ents = [(0, b"")] * 40 + [(1, X.payload(rng, 1 << 20))] + [(0, b"")] * 23
    _check_bytes(ctx, X.Entries([("", 0, 0), ("test_chain_id", 5, 0)], ents))


def test_bytes_around_the_wave_copy_cutoff(ctx):
    rng = random.Random(76)
    c = N.VOTE_EXT_WAVE_MIN
    ents = [(0, X.payload(rng, ln)) for _ in range(3) for ln in (c - 1, c, c + 1, 1, c, 0, c - 1)]
    _check_bytes(ctx, X.Entries([("test_chain_id", 9, 2)], ents))


def test_bad_arguments_rejected(ctx):
    t = [R.tail("c", 1, 0)]
    with pytest.raises(N.NativeError):  # template index out of range
        ctx.vote_extension_sign_bytes_device(t, [1], np.zeros(4, np.uint8), [0, 4])
    with pytest.raises(N.NativeError):  # decreasing offsets
        ctx.vote_extension_sign_bytes_device(t, [0, 0], np.zeros(4, np.uint8), [0, 4, 2])
    with pytest.raises(N.NativeError):  # ext_off[0] != 0
        ctx.vote_extension_sign_bytes_device(t, [0], np.zeros(4, np.uint8), [1, 4])


# ---------------------------------------------------------------- verdicts
def _ed_signer(k):
    return Ed25519Signer(key_seed(k))


def _batch(pks, sigs, msgs):
    return Batch.from_entries(list(zip(pks, msgs, sigs)))


@pytest.fixture(scope="module")
def ed_case():
    """1,500 entries over 25 templates and 97 keys: 750 vote entries, then the
    750 extension entries of the same keys; the oracle's statuses over the
    checker's messages, computed once."""
    rng = random.Random(77)
    vt, votes, sent, pks, sigs, msgs = X.signed_batch(rng, _ed_signer, 25, 750, 97)
    b = _batch(pks, sigs, msgs)
    _, ref = C.ed25519_verify_packed(b.pk, b.sig, b.msg, b.off, threads=8)
    ref.setflags(write=False)
    return vt, votes, sent, b, ref


def _run(ctx, kind, flags, vt, votes, sent, b, nv=None, ne=None):
    """The first nv vote entries and the first ne extension entries of the case."""
    n = len(votes)
    nv = n if nv is None else nv
    ne = len(sent.tmpl) if ne is None else ne
    segs = [V.segments(t) for t in vt]
    pk = np.concatenate([b.pk[:32 * nv], b.pk[32 * n:32 * (n + ne)]])
    sig = np.concatenate([b.sig[:64 * nv], b.sig[64 * n:64 * (n + ne)]])
    return ctx.verify_votes_and_extensions(kind, flags, segs, votes[:nv], sent.tails, sent.tmpl[:ne],
                                           sent.data[:int(sent.off[ne])], sent.off[:ne + 1], pk, sig)


@pytest.mark.parametrize("flags", [N.TMV_FLAG_KEY_CACHE, 0, N.TMV_FLAG_BATCH_EQUATION, N.TMV_FLAG_PER_ENTRY])
def test_statuses_match_oracle(ctx, ed_case, flags):
    vt, votes, sent, b, ref = ed_case
    n = len(votes)
    for half in (ref[:n], ref[n:]):  # the generator yields good and bad entries of both kinds
        assert half.min() == 0 and half.max() == 1
    ok, st = _run(ctx, N.TMV_KIND_ED25519, flags, *ed_case[:4])
    assert np.array_equal(st.astype(np.uint8), ref)
    assert ok == bool(ref.all())
    ok2, st2 = ctx.verify_batch_ex(N.TMV_KIND_ED25519, flags, b.pk, b.sig, b.msg, b.off)  # host-built messages
    assert np.array_equal(st, st2)


def test_one_kind_only_equals_the_one_kind_calls(ctx, ed_case):
    vt, votes, sent, b, ref = ed_case
    n = len(votes)
    _, st = _run(ctx, N.TMV_KIND_ED25519, N.TMV_FLAG_KEY_CACHE, vt, votes, sent, b, ne=0)
    _, want = ctx.verify_votes(N.TMV_KIND_ED25519, N.TMV_FLAG_KEY_CACHE, [V.segments(t) for t in vt], votes,
                               b.pk[:32 * n], b.sig[:64 * n])
    assert np.array_equal(st, want) and np.array_equal(st.astype(np.uint8), ref[:n])
    _, st = _run(ctx, N.TMV_KIND_ED25519, N.TMV_FLAG_KEY_CACHE, vt, votes, sent, b, nv=0)
    lo = int(b.off[n])
    _, want = ctx.verify_batch_ex(N.TMV_KIND_ED25519, N.TMV_FLAG_KEY_CACHE, b.pk[32 * n:], b.sig[64 * n:],
                                  b.msg[lo:], b.off[n:] - b.off[n])
    assert np.array_equal(st, want) and np.array_equal(st.astype(np.uint8), ref[n:])


def test_two_logical_devices_same_statuses(ed_case):
    """Two shards: with 500 vote entries and 750 extension entries the first
    shard holds both kinds and the second starts inside the payloads."""
    vt, votes, sent, b, ref = ed_case
    n = len(votes)
    c2 = N.Context(1, logical=2)
    try:
        for flags in (N.TMV_FLAG_KEY_CACHE, 0):
            _, st = _run(c2, N.TMV_KIND_ED25519, flags, vt, votes, sent, b, nv=500)
            assert np.array_equal(st.astype(np.uint8), np.concatenate([ref[:500], ref[n:]]))
    finally:
        c2.close()


def test_statuses_sr25519(ctx):
    from tendermint_amd.testing.sr25519_factory import Sr25519Signer, mini_from_secret

    class Signer:
        def __init__(self, k):
            self.s = Sr25519Signer(mini_from_secret(b"key: %x" % k))
            self.public_key = self.s.public_key

        def sign(self, m):
            return self.s.sign(m, b"%d" % (len(m) * 131 + m[-1]))

    rng = random.Random(78)
    vt, votes, sent, pks, sigs, msgs = X.signed_batch(rng, Signer, 10, 200, 31, max_len=4096, bad_sig=0.06)
    b = _batch(pks, sigs, msgs)
    ref = C.sr25519_status_packed(b.pk, b.sig, b.msg, b.off, threads=8)
    for half in (ref[:200], ref[200:]):
        assert half.min() != 1 and half.max() == 1
    for flags in (N.TMV_FLAG_KEY_CACHE, 0):
        _, st = _run(ctx, N.TMV_KIND_SR25519, flags, vt, votes, sent, b)
        assert np.array_equal(st, ref)


# ---------------------------------------------------------------- host layer on the device
@pytest.fixture(params=["host-built", "device-built"])
def backend(request, ctx, monkeypatch):
    """tmv_verify_extended_votes of libtmgpu.so, the messages built by the
    host encoder (tmv_verify_batch_ex) or on the device
    (tmv_verify_votes_and_extensions); secp256k1 entries through
    tmv_secp256k1_verify_batch either way."""
    from tendermint_amd import host as H
    monkeypatch.setenv("TMV_VOTE_EXT_DEVICE_MIN", "0" if request.param == "device-built" else "4000000000")
    return lambda mode, chain, votes, keys: H.verify_extended_votes(ctx, mode, chain, votes, keys)


@pytest.fixture(scope="module")
def sig_ok():
    return X.make_sig_ok()


@pytest.fixture(scope="module")
def mode_case(sig_ok):
    table = X.mode_table(X.table_vals())
    return table, {m: X.expected_mode_results(m, table, sig_ok) for m in (0, 1, 2)}


def test_host_layer_mode_table(backend, mode_case):
    X.check_mode_table(backend, *mode_case)


def test_host_layer_extended_commits(backend, sig_ok):
    X.check_extended_commits(backend, sig_ok)
