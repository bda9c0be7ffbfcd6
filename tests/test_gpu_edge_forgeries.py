"""tests/golden/edge_forgeries.json on the device: inputs that are valid if
and only if one named rejection check is skipped (a rejected key or R taken
for the identity its table holds, a rejected encoding of the signer's own
point, S + l, the missing marker) and the valid edges that must be accepted
(the zero sr25519 key, R = identity, points of mixed order).  An honest
signature with a flipped bit fails the equation whatever a kernel does with
its flags; these do not, so each kernel family's own copy of the decision is
what gives the fixture's status: per entry, the batch equation (inside groups
that must pass without falling back), the cached key tables cold, warm and
with the keys swapped, merged keys, mixed batches, the device-resident entry
point and the host layer's BatchVerifier."""
import numpy as np
import pytest

import ed25519_ref as E
import oracle_c as C
import sr25519_ref as S
from tendermint_amd import _native as N
from tendermint_amd.testing.factory import Batch, make_commit_batch, make_sr25519_batch

import edge_forgeries_cases as F
from test_batch_verifier import Backend

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ED, SR = N.TMV_KIND_ED25519, N.TMV_KIND_SR25519
PER, BEQ, KC = N.TMV_FLAG_PER_ENTRY, N.TMV_FLAG_BATCH_EQUATION, N.TMV_FLAG_KEY_CACHE
FLAGS = [PER, BEQ, KC, KC | BEQ]
FLAG_IDS = ["per_entry", "batch_equation", "key_cache", "key_cache+batch_equation"]
KINDS = [ED, SR]
KIND_IDS = ["ed25519", "sr25519"]
M_LOG2 = 6
M = 1 << M_LOG2
ZERO32 = bytes(32)
ED_IDENTITY = b"\x01" + bytes(31)  # y = 1: the ed25519 key that is the identity, as the zero sr25519 key is


@pytest.fixture(scope="module")
def bctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = N.Context(1)
    c.set_batch_options(seed=SEED, stats=True)
    yield c
    c.close()


class Case:
    """One scheme's records as a batch, the honest entries they are spread among, and the oracle."""

    def __init__(self, golden, kind):
        self.kind = kind
        self.vs = F.records(golden, "ed25519" if kind == ED else "sr25519")
        self.recs = Batch.from_entries(F.entries(self.vs))
        self.want = F.statuses(self.vs)
        self.honest = make_commit_batch(1500) if kind == ED else make_sr25519_batch(1500, bad_frac=0.0)
        self.pool = Batch.concat([self.honest, self.recs])  # entry 1500 + i is record i

    def oracle(self, b):
        if self.kind == ED:
            return C.ed25519_verify_packed(b.pk, b.sig, b.msg, b.off, threads=8)[1].astype(np.int8)
        return C.sr25519_status_packed(b.pk, b.sig, b.msg, b.off, threads=8)

    def prechecks(self, b):
        return C.ed25519_prechecks(b.pk, b.sig) if self.kind == ED else C.sr25519_prechecks(b.pk, b.sig)

    def layout(self, at, n, keyed=0):
        """A batch of n entries with record r at position at[r], honest
        entries elsewhere (keyed: only that many honest signers, repeated, so
        that a key-cached batch equation merges keys).  Returns (batch,
        expected statuses)."""
        idx = np.arange(n) % (keyed or self.honest.n)
        want = np.ones(n, np.int8)
        for r, pos in at.items():
            idx[pos] = self.honest.n + r
            want[pos] = self.want[r]
        return self.pool.take(idx), want

    def spread_layouts(self):
        """Every record alone in a group of M once: chunks of 23 records, record
        j of a chunk in group j, at lane 0 or 63 of its group -- lanes 0, 63,
        64 and 127 of a block of 128."""
        per = 23
        for lo in range(0, len(self.vs), per):
            at = {r: M * j + (0 if (j // 2) % 2 == 0 else M - 1)
                  for j, r in enumerate(range(lo, min(lo + per, len(self.vs))))}
            yield at, M * per

    def packed_layout(self):
        """All records together, behind 37 honest entries (so they straddle group edges), honest entries after."""
        return {r: 37 + r for r in range(len(self.vs))}, 1500


_CASES = {}


@pytest.fixture(scope="module")
def case(golden):
    def get(kind):
        if kind not in _CASES:
            _CASES[kind] = Case(golden, kind)
        return _CASES[kind]
    return get


def _run(bctx, kind, flags, b):
    """(statuses, groups, failed groups) of one call with groups of M."""
    bctx.set_batch_options(group_log2=M_LOG2, seed=SEED, stats=True)
    s0 = bctx.batch_stats()
    ok, st = bctx.verify_batch_ex(kind, flags, b.pk, b.sig, b.msg, b.off)
    s1 = bctx.batch_stats()
    assert ok == bool((st == 1).all())
    return st, s1["groups"] - s0["groups"], s1["failed"] - s0["failed"]


def _mismatch(c, at, st, want):
    """The records whose status is not the fixture's (named, for the failure message)."""
    return [(c.vs[r]["name"], c.vs[r]["skipped_check"], int(st[pos]), int(want[pos])) for r, pos in at.items()
            if st[pos] != want[pos]]


def test_fixture_statuses_are_the_oracles(case):
    """The statuses the device is held to are the C oracle's (as the CPU suite checks entry by entry)."""
    for kind in KINDS:
        c = case(kind)
        assert np.array_equal(c.oracle(c.recs), c.want)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_every_path_inside_working_groups(bctx, case, kind, flags):
    """Every record through every flag set, alone in a group of honest
    entries and then all packed together: each status is the fixture's and
    each honest entry stays valid.  Every record that is not valid fails a
    pre-check, so under the batch equation no group may fail and fall back:
    the rejected entries are left out of the sums, and the mixed-order and
    identity entries are in them and pass the cofactored equation."""
    c = case(kind)
    layouts = list(c.spread_layouts()) + [c.packed_layout()]
    if flags == KC | BEQ:  # few honest keys: the key-cached batch equation merges them
        layouts += [(at, n, 40) for at, n in layouts[-2:]]
    for at, n, *keyed in layouts:
        b, want = c.layout(at, n, *keyed)
        st, groups, failed = _run(bctx, kind, flags, b)
        assert not _mismatch(c, at, st, want)
        assert np.array_equal(st, want)
        if flags & BEQ and groups:
            assert groups == (n + M - 1) // M
            pre = c.prechecks(b)
            assert failed == C.failing_groups(pre, want == 1, M) == 0
            assert not (pre & (want != 1)).any() and (pre | (want != 1)).all()


def _with_bad_honest(c, at, n, keyed=0):
    """The layout with one honest entry per group made invalid behind passing
    pre-checks (S's low bit flipped), in every group that holds an honest
    entry: those groups fail the equation and are decided again by the
    fallback kernels."""
    b, want = c.layout(at, n, keyed)
    sig, want, taken = b.sig.copy(), want.copy(), set(at.values())
    for g in range(0, n, M):
        pos = next((q for q in range(g + 5, min(g + M, n)) if q not in taken), None)
        if pos is not None:
            sig[64 * pos + 32] ^= 0x01
            want[pos] = 0
    b = Batch(b.pk, sig, b.msg, b.off)
    assert np.array_equal(c.oracle(b), want)
    return b, want


@pytest.mark.parametrize("path", ["fallback", "located", "merged_fallback"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_failing_groups_keep_the_verdicts(bctx, case, kind, path, monkeypatch):
    """The records inside groups that do fail (one honest entry per group
    with S's low bit flipped): the whole group is verified again one by one
    (`fallback`; `merged_fallback`: against the cached key tables), or the
    index-weighted second pass names the one bad entry and only that one is
    verified (`located`, TMV_LOCATE_MIN read at every launch).  Each of these
    kernels decides on its own what a rejected key, R or scalar gives; the
    statuses are the fixture's and exactly the groups with a flipped entry
    fail."""
    monkeypatch.setenv("TMV_LOCATE_MIN", "1000" if path == "located" else "0")
    c = case(kind)
    flags, keyed = (KC | BEQ, 40) if path == "merged_fallback" else (BEQ, 0)
    for at, n in (next(iter(c.spread_layouts())), c.packed_layout()):
        b, want = _with_bad_honest(c, at, n, keyed)
        bctx.metrics_reset()
        st, groups, failed = _run(bctx, kind, flags, b)
        met = bctx.metrics()
        assert not _mismatch(c, at, st, want)
        assert np.array_equal(st, want)
        n_bad = int((want == 0).sum()) - sum(1 for r in at if c.want[r] == 0)
        assert groups == (n + M - 1) // M and n_bad >= groups - 3
        if path == "merged_fallback":  # its groups are of the entries in key order: the flipped ones fall elsewhere
            assert 1 <= failed <= n_bad
            continue
        assert failed == C.failing_groups(c.prechecks(b), want == 1, M) == n_bad
        if path == "located":
            assert (met["located_groups"], met["fallback_signatures"]) == (n_bad, n_bad)
        elif path == "fallback":
            # whole groups, not single entries (entries the pre-checks decided need no second look)
            assert met["located_groups"] == 0 and 8 * n_bad < met["fallback_signatures"] <= n


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_merged_path_is_taken(bctx, case, kind):
    """The keyed layouts of the sweep above do take the key-merged batch
    equation (few keys per group), and the layouts of 1500 honest keys do not."""
    c = case(kind)
    at, n = c.packed_layout()
    for keyed, merged in ((40, True), (0, False)):
        b, want = c.layout(at, n, keyed)
        st, groups, failed = _run(bctx, kind, KC | BEQ, b)
        assert np.array_equal(st, want)
        assert (groups > 0) == merged and failed == 0


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_unflagged_entry_points(ctx, case, kind):
    c = case(kind)
    at, n = c.packed_layout()
    b, want = c.layout(at, n)
    if kind == ED:
        ok, st = ctx.ed25519_verify_batch(b.pk, b.sig, b.msg, b.off)
    else:
        ok, st = ctx.sr25519_verify_batch(b.pk, b.sig, b.msg, b.off)
    assert not ok and not _mismatch(c, at, st.astype(np.int8), want)
    assert np.array_equal(st.astype(np.int8), want)
    # the records alone, no honest entry around them
    if kind == ED:
        ok, st = ctx.ed25519_verify_batch(c.recs.pk, c.recs.sig, c.recs.msg, c.recs.off)
    else:
        ok, st = ctx.sr25519_verify_batch(c.recs.pk, c.recs.sig, c.recs.msg, c.recs.off)
    assert not ok and np.array_equal(st.astype(np.int8), c.want)


def test_ed25519_one_at_a_time(ctx, case):
    c = case(ED)
    got = [int(ctx.ed25519_verify(*F.entry(v))) for v in c.vs]
    assert [(v["name"], g) for v, g in zip(c.vs, got) if g != v["status"]] == []


def _swap_keys(c, keyed=0):
    """The packed layout with the keys swapped between the entries that hold a
    rejected key beside R = [s]B and those that hold the identity key: the
    first become valid, the second rejected.  Both keys' cached tables hold
    the identity; only their ok bytes tell them apart."""
    at, n = c.packed_layout()
    b, want = c.layout(at, n, keyed)
    pk = b.pk.copy()
    ident = ZERO32 if c.kind == SR else ED_IDENTITY
    head = "key_identity" if c.kind == SR else "a_identity"
    rejected = bytes.fromhex(next(v for v in c.vs if F.name_parts(v)[0] == head)["pk"])
    flipped = {}
    for r, v in enumerate(c.vs):
        if F.name_parts(v)[0] == head:                      # R = [s]B under the identity key: valid
            new, flipped[at[r]] = ident, 1
        elif v["pk"] == ident.hex():                        # whatever it held, now under a rejected key
            new, flipped[at[r]] = rejected, (-1 if c.kind == SR else 0)
        else:
            continue
        pk[32 * at[r]:32 * at[r] + 32] = np.frombuffer(new, np.uint8)
    want = want.copy()
    for pos, s in flipped.items():
        want[pos] = s
    return Batch(pk, b.sig, b.msg, b.off), want, len(flipped)


@pytest.mark.parametrize("flags", [KC, KC | PER, KC | BEQ],
                         ids=["key_cache", "key_cache+per_entry", "key_cache+batch_eq"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_key_cache_cold_warm_swapped(case, kind, flags):
    """On a context of its own: the first call builds the key tables (a
    rejected key's is the identity, with ok = 0), the second reads them, and
    the third has the rejected and the identity keys swapped between entries,
    so that a consumer that forgot the ok byte -- or kept it by entry instead
    of by key -- gives another vector."""
    c = case(kind)
    at, n = c.packed_layout()
    keyed = 40 if flags & BEQ else 0
    b, want = c.layout(at, n, keyed)
    swapped, want_swapped, n_swapped = _swap_keys(c, keyed)
    assert n_swapped >= 30 and np.array_equal(c.oracle(swapped), want_swapped)
    own = N.Context(1)
    try:
        own.set_batch_options(group_log2=M_LOG2, seed=SEED, stats=True)
        h0 = own.key_cache_stats()
        for call in ("cold", "warm"):
            ok, st = own.verify_batch_ex(kind, flags, b.pk, b.sig, b.msg, b.off)
            assert not _mismatch(c, at, st, want), call
            assert np.array_equal(st, want), call
        h1 = own.key_cache_stats()
        assert h1["misses"] > h0["misses"] and h1["hits"] > h0["hits"]
        ok, st = own.verify_batch_ex(kind, flags, swapped.pk, swapped.sig, swapped.msg, swapped.off)
        assert np.array_equal(st, want_swapped)
        ok, st = own.verify_batch_ex(kind, flags, b.pk, b.sig, b.msg, b.off)
        assert np.array_equal(st, want)
    finally:
        own.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_merged_rejected_and_identity_keys(bctx, case, kind):
    """One rejected key and the identity key, each on 40 entries of one group
    of 128 with R = [s_i]B, beside 48 entries of four honest keys, under the
    key-merged batch equation: the rejected key's run is left out of the sums
    (all -1; ed25519: 0), the identity key's run is in them (all 1), and the
    group passes."""
    c = case(kind)
    head = "key_identity" if kind == SR else "a_identity"
    rejected = bytes.fromhex(next(v for v in c.vs if F.name_parts(v)[0] == head)["pk"])
    ident = ZERO32 if kind == SR else ED_IDENTITY
    ents, want = [], []
    for i in range(80):
        s = (0x1234567 * (i + 1)) ** 7 % E.L
        sB = E.pt_mul(s, E.BASE)
        sb = bytearray(s.to_bytes(32, "little"))
        if kind == SR:
            sb[31] |= 0x80
        Rb = S.ristretto_encode(sB) if kind == SR else E.pt_encode(sB)
        bad = i % 2 == 0
        ents.append((rejected if bad else ident, b"merged %d" % i, Rb + bytes(sb)))
        want.append((-1 if kind == SR else 0) if bad else 1)
    ents += [c.honest.entry(i % 4) for i in range(48)]
    want = np.array(want + [1] * 48, np.int8)
    b = Batch.from_entries(ents)
    assert np.array_equal(c.oracle(b), want)
    bctx.set_batch_options(group_log2=7, seed=SEED, stats=True)
    try:
        s0 = bctx.batch_stats()
        ok, st = bctx.verify_batch_ex(kind, KC | BEQ, b.pk, b.sig, b.msg, b.off)
        s1 = bctx.batch_stats()
    finally:
        bctx.set_batch_options(seed=SEED, stats=True)
    assert np.array_equal(st, want) and not ok
    assert (s1["groups"] - s0["groups"], s1["failed"] - s0["failed"]) == (1, 0)


def _interleaved(case):
    """ed25519 and sr25519 records alternately (the longer list's tail after)."""
    ed, sr = case(ED), case(SR)
    ents, kinds, want, names = [], [], [], []
    for i in range(max(len(ed.vs), len(sr.vs))):
        for k, c in ((ED, ed), (SR, sr)):
            if i < len(c.vs):
                ents.append(F.entry(c.vs[i]))
                kinds.append(k)
                want.append(c.vs[i]["status"])
                names.append(c.vs[i]["name"])
    return Batch.from_entries(ents), np.array(kinds, np.uint8), np.array(want, np.int8), names


@pytest.mark.parametrize("n", [1, 63, 64, 65, 0], ids=["1", "63", "64", "65", "all"])
def test_mixed_batches(ctx, case, n):
    b, kinds, want, names = _interleaved(case)
    n = n or b.n
    b, kinds, want = b.take(np.arange(n)), kinds[:n].copy(), want[:n]
    ok, st = ctx.verify_mixed_batch(kinds, b.pk, b.sig, b.msg, b.off)
    assert [(names[i], int(st[i]), int(want[i])) for i in range(n) if st[i] != want[i]] == []
    assert ok == bool((want == 1).all())
    for flags in (PER, BEQ):
        ok, st = ctx.verify_mixed_batch_ex(flags, kinds, b.pk, b.sig, b.msg, b.off)
        assert np.array_equal(st, want), flags


def test_mixed_device_resident(ctx, case):
    import torch
    b, kinds, want, names = _interleaved(case)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).to(dev) for k in ("pk", "sig", "msg")}
    off = torch.from_numpy(b.off.view(np.int32)).to(dev)
    dk = torch.from_numpy(kinds).to(dev)
    out = torch.full((b.n,), -7, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    ctx.verify_mixed_batch_device(0, dk.data_ptr(), t["pk"].data_ptr(), t["sig"].data_ptr(), t["msg"].data_ptr(),
                                  off.data_ptr(), b.n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = out.cpu().numpy()
    assert [(names[i], int(st[i]), int(want[i])) for i in range(b.n) if st[i] != want[i]] == []


def test_batch_verifier_rejected_keys_gpu(ctx, golden):
    F.check_batch_verifier_rejected_keys(Backend(ctx.handle, None), golden)
