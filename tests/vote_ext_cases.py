"""Shared case tables for the vote-extension tests: extension entries for
the device builder (k_vote_ext_signbytes) with their expected messages from
the checker (vote_ext_ref.py), and signed vote + extension batches."""
from __future__ import annotations

import random

import numpy as np

import vote_cases as V
import vote_ext_ref as R

# payload lengths around every unit the kernel moves (byte, dword, 16 bytes,
# a wave's 256 bytes) and around one-, two- and three-byte length varints
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 4095, 4097]
BOUNDARY_TEMPLATE = ("test_chain_id", 1, 1)
# len(body) = 127 / 128 and 16383 / 16384 for BOUNDARY_TEMPLATE
BOUNDARY_LENGTHS = [92, 93, 16347, 16348]
# every combination of empty and non-empty height / round / chain_id
TAIL_COMBOS = [(c, h, r) for c in ("", "test_chain_id") for h in (0, 7) for r in (0, 3)]


def payload(rng: random.Random, n: int) -> bytes:
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def random_template(rng: random.Random):
    return (rng.choice(V.CHAIN_IDS + ["test_chain_id"] * 3), rng.choice(V.HEIGHTS + [rng.randrange(1, 1 << 40)] * 3),
            rng.choice(V.ROUNDS + [0] * 3))


class Entries:
    """Extension entries: templates (chain_id, height, round) and (template
    index, payload) pairs -> the engine's arrays and the checker's messages."""

    def __init__(self, templates, entries):
        self.templates, self.entries = templates, entries
        self.tails = [R.tail(*t) for t in templates]
        self.tmpl = np.array([t for t, _ in entries], np.uint32)
        data, off = R.concat([p for _, p in entries])
        self.data = np.frombuffer(data, np.uint8) if data else np.zeros(0, np.uint8)
        self.off = np.array(off, np.uint32)
        self.msgs = [R.sign_bytes(*templates[t], p) for t, p in entries]

    def expected(self):
        msg, off = R.concat(self.msgs)
        return msg, np.array(off, np.uint32)


def random_entries(rng: random.Random, n_tmpl: int, n: int, max_len: int = 300) -> Entries:
    tmpls = [random_template(rng) for _ in range(n_tmpl)]
    ents = []
    for _ in range(n):
        k = rng.randrange(6)
        ln = 0 if k == 0 else rng.randrange(1, 40) if k < 4 else rng.randrange(40, max_len + 1)
        ents.append((rng.randrange(n_tmpl), payload(rng, ln)))
    return Entries(tmpls, ents)


def length_offset_entries(rng: random.Random) -> Entries:
    """Every length of LENGTHS at all 16 source offsets mod 16 (a filler entry
    in front of each moves the source offset)."""
    tmpls = [random_template(rng) for _ in range(5)]
    ents, at = [], 0
    for ln in LENGTHS:
        for r in range(16):
            fill = (r - at) % 16
            ents.append((rng.randrange(5), payload(rng, fill)))
            at += fill
            assert at % 16 == r
            ents.append((rng.randrange(5), payload(rng, ln)))
            at += ln
    return Entries(tmpls, ents)


def signed_batch(rng: random.Random, signer_of, n_tmpl: int, n_pairs: int, n_keys: int, max_len: int = 300,
                 bad_sig: float = 0.05, bad_ext: float = 0.02):
    """n_pairs vote entries and n_pairs extension entries of the same keys.
    Returns (vote templates, votes, Entries as sent, pk list, sig list,
    messages as signed over: vote messages then the extension messages of
    the payloads as sent).  bad_sig of all signatures get one bit flipped,
    bad_ext of the extension payloads one byte flipped after signing."""
    vt, votes, vmsgs = V.random_votes(rng, n_tmpl, n_pairs)
    sent = random_entries(rng, n_tmpl, n_pairs, max_len)
    pks, sigs = [], []
    signed = vmsgs + sent.msgs
    for i, m in enumerate(signed):
        s = signer_of(i % n_pairs % n_keys)
        sig = s.sign(m)
        if rng.random() < bad_sig:
            b = bytearray(sig)
            b[rng.randrange(64)] ^= 1 << rng.randrange(8)
            sig = bytes(b)
        pks.append(s.public_key)
        sigs.append(sig)
    ents = list(sent.entries)
    for j, (t, p) in enumerate(ents):
        if p and rng.random() < bad_ext:
            b = bytearray(p)
            b[rng.randrange(len(p))] ^= 0x40
            ents[j] = (t, bytes(b))
    sent = Entries(sent.templates, ents)
    return vt, votes, sent, pks, sigs, vmsgs + sent.msgs


# ---------------------------------------------------------------- host layer: validators, votes, extended commits
import hashlib  # noqa: E402

from tendermint_amd import host as H  # noqa: E402
from tendermint_amd.types.canonical import BlockID as CBID, PartSetHeader, Timestamp, vote_sign_bytes  # noqa: E402

CHAIN = "test_chain_id"
BLOCK = H.BlockID(b"\x21" * 32, 3, b"\x22" * 32)


class Val:
    """A validator key of one kind with the address the reference derives."""

    def __init__(self, kind: int, i: int):
        self.kind = kind
        if kind == R.KIND_ED25519:
            from tendermint_amd.testing._openssl import Ed25519Signer
            s = Ed25519Signer(hashlib.sha256(b"ve key %d" % i).digest())
            self._sign = s.sign
        elif kind == R.KIND_SR25519:
            from tendermint_amd.testing.sr25519_factory import Sr25519Signer, mini_from_secret
            s = Sr25519Signer(mini_from_secret(b"ve key: %x" % i))
            self._sign = lambda m: s.sign(m, hashlib.sha256(m).digest())
        else:
            from tendermint_amd.testing.secp256k1_factory import Secp256k1Signer
            s = Secp256k1Signer.from_secret(b"ve secp: %x" % i)
            self._sign = s.sign
        self.pub_key = s.public_key
        self.address = R.key_address(kind, self.pub_key)
        self.key = (kind, self.pub_key)

    def sign(self, m: bytes) -> bytes:
        return self._sign(m)


def vote_msg(chain: str, v: H.Vote) -> bytes:
    """VoteSignBytes from the mirror pinned by the reference's vectors."""
    b = v.block_id
    bid = CBID(b.hash, PartSetHeader(b.psh_total, b.psh_hash)) if (b.hash or b.psh_total or b.psh_hash) else None
    return vote_sign_bytes(chain, v.type, v.height, v.round, bid, Timestamp(*v.timestamp))


def signed_vote(val: Val, idx: int, vtype=H.PRECOMMIT_TYPE, bid=BLOCK, ext=b"", height=1, round_=0,
                ts=(1600000000, 0), chain=CHAIN, sign_ext=None) -> H.Vote:
    """What a privval returns (privval/file.go signVote): the vote signature,
    and for a non-nil precommit the extension signature."""
    v = H.Vote(vtype, height, round_, bid, ts, val.address, idx, b"", ext, b"")
    v.signature = val.sign(vote_msg(chain, v))
    nil = not (bid.hash or bid.psh_total or bid.psh_hash)
    if sign_ext if sign_ext is not None else (vtype == H.PRECOMMIT_TYPE and not nil):
        v.extension_signature = val.sign(R.sign_bytes(chain, height, round_, ext))
    return v


def as_dict(v: H.Vote) -> dict:
    b = v.block_id
    return dict(type=v.type, height=v.height, round=v.round, block_id=(b.hash, b.psh_total, b.psh_hash),
                validator_address=v.validator_address, signature=v.signature, extension=v.extension,
                extension_signature=v.extension_signature, timestamp=v.timestamp)


def make_sig_ok():
    import oracle_c as C
    import secp256k1_ref as S

    def sig_ok(kind, pk, msg, sig):
        if len(sig) != 64:
            return False
        if kind == R.KIND_ED25519:
            return len(pk) == 32 and bool(C.ed25519_verify(pk, msg, sig))
        if kind == R.KIND_SR25519:
            return len(pk) == 32 and bool(C.sr25519_verify(pk, msg, sig))
        return len(pk) == 33 and bool(S.verify(pk, msg, sig))
    return sig_ok


def _flip(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def mode_table(vals):
    """Votes of every vote type x nil / non-nil block x what can be wrong, the
    validators taken in turn: [(label, vote, key)]."""
    out, k = [], 0
    for vtype in (H.PREVOTE_TYPE, H.PRECOMMIT_TYPE):
        for bid in (H.BlockID(), BLOCK):
            for label in ("good", "vote sig", "ext sig", "ext byte", "ext sig empty", "ext sig 63", "ext sig 65",
                          "address", "vote sig 63", "no ext", "big ext"):
                val = vals[k % len(vals)]
                ext = b"" if label == "no ext" else b"x" * 5000 if label == "big ext" else b"extension %d" % k
                v = signed_vote(val, k % len(vals), vtype, bid, ext, height=1 + k % 3, round_=k % 2,
                                ts=(1600000000 + k, k), sign_ext=True)
                if label == "vote sig":
                    v.signature = _flip(v.signature, 7)
                elif label == "ext sig":
                    v.extension_signature = _flip(v.extension_signature, 40)
                elif label == "ext byte":
                    v.extension = _flip(v.extension, 2)
                elif label == "ext sig empty":
                    v.extension_signature = b""
                elif label == "ext sig 63":
                    v.extension_signature = v.extension_signature[:63]
                elif label == "ext sig 65":
                    v.extension_signature += b"\0"
                elif label == "address":
                    v.validator_address = _flip(v.validator_address, 0)
                elif label == "vote sig 63":
                    v.signature = v.signature[:63]
                out.append(("%s/%d/%s" % (label, vtype, "nil" if bid == H.BlockID() else "block"), v, val.key))
                k += 1
    return out


def expected_mode_results(mode: int, table, sig_ok):
    return [R.check_vote(mode, CHAIN, as_dict(v), key[0], key[1], sig_ok, vote_msg(CHAIN, v)) for _, v, key in table]


def extended_commit_cases():
    """Seven validators (five ed25519, one sr25519, one secp256k1) and eight
    extended commits: (validator set, [(label, extended commit)])."""
    vals = [Val(R.KIND_ED25519, i) for i in range(5)] + [Val(R.KIND_SR25519, 5), Val(R.KIND_SECP256K1, 6)]
    vals.sort(key=lambda v: v.address)
    vset = H.ValidatorSet([H.Validator(v.address, v.pub_key, 10, v.kind) for v in vals], proposer_index=0)

    def commit(height, absent=(), nil=()):
        sigs = []
        for i, val in enumerate(vals):
            if i in absent:
                sigs.append(H.ExtendedCommitSig())
                continue
            bid = H.BlockID() if i in nil else BLOCK
            v = signed_vote(val, i, H.PRECOMMIT_TYPE, bid, b"" if i in nil else b"ext %d/%d" % (height, i), height=height,
                            ts=(1600000000 + i, 0))
            sigs.append(H.ExtendedCommitSig(H.BLOCK_ID_FLAG_NIL if i in nil else H.BLOCK_ID_FLAG_COMMIT, val.address,
                                            v.timestamp, v.signature, v.extension, v.extension_signature))
        return H.ExtendedCommit(height, 0, BLOCK, sigs)

    cases = [("good", commit(10))]
    c = commit(11)
    c.extended_signatures[2].extension_signature = _flip(c.extended_signatures[2].extension_signature, 3)
    cases.append(("bad extension signature", c))
    c = commit(12)
    c.extended_signatures[4].signature = _flip(c.extended_signatures[4].signature, 63)
    cases.append(("bad vote signature", c))
    c = commit(13)
    c.extended_signatures[1].extension, c.extended_signatures[1].extension_signature = b"", b""
    cases.append(("missing extension signature", c))
    cases.append(("absent entry", commit(14, absent=(3,))))
    cases.append(("too little power", commit(15, absent=(0, 2, 4, 6))))
    cases.append(("height 0", commit(0)))
    cases.append(("nil entry", commit(17, nil=(5,))))
    return vals, vset, cases


def checker_commit(ec: H.ExtendedCommit) -> dict:
    b = ec.block_id
    return dict(height=ec.height, round=ec.round, block_id=(b.hash, b.psh_total, b.psh_hash),
                sigs=[dict(flag=s.block_id_flag, validator_address=s.validator_address, timestamp=tuple(s.timestamp),
                           signature=s.signature, extension=s.extension, extension_signature=s.extension_signature)
                      for s in ec.extended_signatures])


def checker_vote_msg(chain: str):
    def f(v: dict) -> bytes:
        b = v["block_id"]
        bid = None if R.block_id_is_nil(b) else CBID(b[0], PartSetHeader(b[1], b[2]))
        return vote_sign_bytes(chain, v["type"], v["height"], v["round"], bid, Timestamp(*v["timestamp"]))
    return f


# ---------------------------------------------------------------- checks shared by the CPU and the GPU suite
# backend(mode, chain_id, votes, keys) -> [(TMV_VOTE_*, failed signature)]: the CPU harness or the device
def table_vals():
    return [Val(R.KIND_ED25519, 20), Val(R.KIND_ED25519, 21), Val(R.KIND_SR25519, 22), Val(R.KIND_SECP256K1, 23),
            Val(R.KIND_ED25519, 24)]


def check_mode_table(backend, table, expected_by_mode):
    """The table through the backend in every mode equals the checker, and
    every outcome occurs."""
    votes, keys = [v for _, v, _ in table], [k for _, _, k in table]
    seen = set()
    for mode in (R.MODE_VERIFY, R.MODE_VERIFY_AND_EXTENSION, R.MODE_EXTENSION):
        got = backend(mode, CHAIN, votes, keys)
        want = expected_by_mode[mode]
        for (label, _, _), g, w in zip(table, got, want):
            assert tuple(g) == tuple(w), "mode %d, %s" % (mode, label)
        seen |= set(map(tuple, want))
    assert seen == {(R.OK, 0), (R.ERR_ADDRESS, 0), (R.ERR_SIGNATURE, 1), (R.ERR_SIGNATURE, 2)}


def vote_and_extension(backend):
    """The VerifyFn of an extended VoteSet over a backend, counting its calls."""
    def f(chain, votes, keys):
        f.calls += 1
        return [r for r, _ in backend(R.MODE_VERIFY_AND_EXTENSION, chain, votes, keys)]
    f.calls = 0
    return f


def check_extended_commits(backend, sig_ok):
    """extended_commits_to_vote_sets over the eight commits: the checker's text
    or a vote set with the checker's majority and votes, in one verify call."""
    from tendermint_amd.vote_set import VoteSet, extended_commits_to_vote_sets
    vals, vset, cases = extended_commit_cases()
    verify = vote_and_extension(backend)
    out = extended_commits_to_vote_sets([(CHAIN, vset, ec) for _, ec in cases], verify)
    assert verify.calls == 1
    cvals = [(v.kind, v.pub_key, v.address, 10) for v in vals]
    texts = {}
    for (label, ec), got in zip(cases, out):
        err, maj, added = R.to_extended_vote_set(CHAIN, cvals, checker_commit(ec), sig_ok, checker_vote_msg(CHAIN))
        if err is not None:
            assert got == err, label
            texts[label] = err
            continue
        assert isinstance(got, VoteSet), "%s: %r" % (label, got)
        assert got.has_two_thirds_majority() and (got.maj23.hash, got.maj23.psh_total, got.maj23.psh_hash) == maj
        assert [i for i, v in enumerate(got.votes) if v is not None] == added
    assert sorted(texts) == ["bad extension signature", "bad vote signature", "height 0",
                             "missing extension signature", "too little power"]
    assert texts["bad extension signature"].endswith(": invalid signature")
    return texts
