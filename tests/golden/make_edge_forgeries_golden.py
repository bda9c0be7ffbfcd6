#!/usr/bin/env python3
"""Writes tests/golden/edge_forgeries.json: ed25519 and sr25519 inputs that are
valid if and only if ONE named rejection check is skipped, and the valid edges
that must be accepted.

An honest signature with a flipped bit fails the group equation whatever the
verifier does with its rejection checks, so it cannot tell a verifier that
skips one from a verifier that keeps it.  Every record here with a
`skipped_check` is built so that the equation holds once that one check is
gone: a rejected key with R = [s]B verifies as soon as the rejected point is
taken for the identity (what a cached key table holds for it) and its `ok`
flag is forgotten; the negative or negative-t encoding of a signer's own point
verifies as soon as the sign test is dropped; S + l verifies as soon as S < l
is.  For each such record the generator asserts

  1. the restatement (oracle/ed25519_ref.py, oracle/sr25519_ref.py) gives the
     stored status, and
  2. a lax verifier -- the same integer formulas below with only that check
     removed -- accepts the entry (status 1).

The `order_*` tags pin the order of the checks (key, then scalar, then R)
instead: there the lax verifier runs the checks in the other order and must
give a different status from the stored one.

`skipped_check` is null on the must-accept records (status 1): the zero
sr25519 key, R = identity, S = l - 1, and ed25519 keys and R of mixed order
(a prime-order point plus a torsion point), valid under ZIP-215's cofactored
equation.

Uses oracle/ed25519_ref.py, oracle/sr25519_ref.py and Python integers only.
The sr25519 verdicts are the restatement's: the reference holds no vector for
them, and accepting the zero key (the Ristretto identity) is the
restatement's reading of schnorrkel.

    python tests/golden/make_edge_forgeries_golden.py
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import ed25519_ref as E  # noqa: E402
import sr25519_ref as S  # noqa: E402

P, L, D = E.P, E.L, E.D
MASK255 = (1 << 255) - 1
ZERO32 = bytes(32)
records = []
SEED = 0xF0261E5
rng = random.Random(SEED)


def b32(x: int) -> bytes:
    return x.to_bytes(32, "little")


# ---------------------------------------------------------------- Ristretto, with one test removable

def sqrt_outcome(w: int) -> str:
    """Which of sqrt_ratio_i(1, w)'s four outcomes w takes: v r^2 is 1
    (`correct`), -1 (`flipped`), -i (`flipped_i`) or +i (`none`)."""
    w %= P
    w3 = w * w % P * w % P
    w7 = w3 * w3 % P * w % P
    r = w3 * pow(w7, (P - 5) // 8, P) % P
    check = w * r % P * r % P
    for label, want in (("correct", 1), ("flipped", P - 1), ("flipped_i", (-E.SQRT_M1) % P), ("none", E.SQRT_M1)):
        if check == want:
            return label
    raise AssertionError("v r^2 is no fourth root of unity")


def rist_decode(b: bytes, skip=None):
    """(point, None) or (None, the first test that fails), the tests in the
    restatement's order: bit255, noncanonical, negative, nonsquare, neg_t,
    y_zero.  `skip` names one test to leave out (a tuple: several)."""
    skip = (skip,) if isinstance(skip, str) else (skip or ())
    s = int.from_bytes(b, "little")
    if s >> 255:
        if "bit255" not in skip:
            return None, "bit255"
        s &= MASK255
    if s >= P:
        return None, "noncanonical"
    if s & 1 and "negative" not in skip:
        return None, "negative"
    ss = s * s % P
    u1 = (1 - ss) % P
    u2 = (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 % P * u1) - u2_sqr) % P
    ok, inv = S.sqrt_ratio_i(1, v * u2_sqr % P)
    if not ok:
        return None, "nonsquare"
    dx = inv * u2 % P
    dy = inv * dx % P * v % P
    x = S._abs(2 * s * dx)
    y = u1 * dy % P
    t = x * y % P
    if t & 1 and "neg_t" not in skip:
        return None, "neg_t"
    if y == 0:
        return None, "y_zero"
    return (x, y, 1, t), None


def rist_class(b: bytes) -> str:
    """`valid`, or the rejection class; non-squares carry sqrt_ratio_i's outcome."""
    pt, why = rist_decode(b)
    if pt is not None:
        return "valid"
    if why == "nonsquare":
        s = int.from_bytes(b, "little")
        ss = s * s % P
        u1, u2 = (1 - ss) % P, (1 + ss) % P
        w = (-(D * u1 % P * u1) - u2 * u2) % P * u2 % P * u2 % P
        assert pow(w, (P - 1) // 2, P) == P - 1, "Euler's criterion disagrees with sqrt_ratio_i"
        label = sqrt_outcome(w)
        assert label in ("flipped_i", "none")
        return "nonsquare_" + label
    return why


def key_sqrt_outcome(b: bytes) -> str:
    """sqrt_ratio_i's outcome while decoding a valid encoding (`correct` or `flipped`)."""
    s = int.from_bytes(b, "little")
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    w = (-(D * u1 % P * u1) - u2 * u2) % P * u2 % P * u2 % P
    assert pow(w, (P - 1) // 2, P) == 1
    label = sqrt_outcome(w)
    assert label in ("correct", "flipped")
    return label


SR_SKIPS = ("key_ok", "key_sign", "key_neg_t", "key_bit255", "r_ok", "s_lt_l", "marker",
            "order_scalar_first", "order_r_first")


def sr_status(pk: bytes, msg: bytes, sig: bytes, skip=None) -> int:
    """BatchVerifier status of one sr25519 entry: 1 valid, 0 invalid, -1 Add
    error on the key, -2 Add error on the signature; checked key, scalar, R."""
    assert skip is None or skip in SR_SKIPS
    A, _ = rist_decode(pk, {"key_sign": "negative", "key_neg_t": "neg_t", "key_bit255": "bit255"}.get(skip))
    if A is None and skip == "key_ok":
        A = E.IDENT  # the table a rejected key leaves behind, its ok flag forgotten
    s = int.from_bytes(sig[32:], "little") & MASK255
    sig_bad = (sig[63] & 0x80 == 0 and skip != "marker") or (s >= L and skip != "s_lt_l")
    R, _ = rist_decode(sig[:32])
    if R is None and skip == "r_ok":
        R = E.IDENT
    order = {"order_scalar_first": "skr", "order_r_first": "krs"}.get(skip, "ksr")
    for c in order:
        if c == "k" and A is None:
            return -1
        if c == "s" and sig_bad:
            return -2
        if c == "r" and R is None:
            return 0
    k = S.challenge(pk, sig[:32], msg)
    Rp = E.pt_add(E.pt_mul(s, E.BASE), E.pt_neg(E.pt_mul(k, A)))
    return 1 if S.ristretto_equal(Rp, R) else 0


def sr_restated(pk: bytes, msg: bytes, sig: bytes) -> int:
    try:
        S.batch_add_check(pk, sig)
    except S.AddError as e:
        return -1 if "public key" in str(e) else -2
    return 1 if S.verify(pk, msg, sig) else 0


# ---------------------------------------------------------------- ed25519, with one test removable

ED_SKIPS = ("a_decode", "r_decode", "s_lt_l")


def ed_status(pk: bytes, msg: bytes, sig: bytes, skip=None) -> int:
    assert skip is None or skip in ED_SKIPS
    Sv = int.from_bytes(sig[32:], "little")
    if Sv >= L and skip != "s_lt_l":
        return 0
    A = E.decode_point_zip215(pk)
    if A is None:
        if skip != "a_decode":
            return 0
        A = E.IDENT
    R = E.decode_point_zip215(sig[:32])
    if R is None:
        if skip != "r_decode":
            return 0
        R = E.IDENT
    k = E.sha512_modl(sig[:32], pk, msg)
    Q = E.pt_add(E.pt_mul(Sv, E.BASE), E.pt_neg(E.pt_add(R, E.pt_mul(k, A))))
    return 1 if E.pt_is_identity(E.pt_mul(8, Q)) else 0


def emit(scheme: str, name: str, skipped, pk: bytes, msg: bytes, sig: bytes, status: int):
    assert len(pk) == 32 and len(sig) == 64
    if scheme == "sr25519":
        strict, restated = sr_status(pk, msg, sig), sr_restated(pk, msg, sig)
        lax = sr_status(pk, msg, sig, skipped) if skipped else None
    else:
        strict, restated = ed_status(pk, msg, sig), int(E.verify_zip215(pk, msg, sig))
        lax = ed_status(pk, msg, sig, skipped) if skipped else None
    assert strict == restated == status, (name, strict, restated, status)
    if skipped is None:
        assert status == 1, (name, "a record without a skipped check is a must-accept one")
    elif skipped.startswith("order_"):
        assert lax != status, (name, "the other order of the checks gives the same status")
    else:
        assert status != 1 and lax == 1, (name, "not accepted with the check removed", skipped, lax)
    assert all(r["name"] != name or r["scheme"] != scheme for r in records), name
    records.append({"scheme": scheme, "name": name, "skipped_check": skipped, "pk": pk.hex(), "msg": msg.hex(),
                    "sig": sig.hex(), "status": status})


def next_msg() -> bytes:
    return b"edge %d" % len(records) + bytes(rng.randrange(256) for _ in range(rng.randrange(6)))


# ---------------------------------------------------------------- sr25519

def sr_sig(R_bytes: bytes, s: int, marker: bool = True) -> bytes:
    b = bytearray(b32(s))
    assert b[31] & 0x80 == 0
    if marker:
        b[31] |= 0x80
    return R_bytes + bytes(b)


def sr_base_sig(s: int) -> bytes:
    """R = [s]B beside s: valid for any key that acts as the identity."""
    return sr_sig(S.ristretto_encode(E.pt_mul(s, E.BASE)), s)


class Signer:
    def __init__(self, i: int):
        self.mini = S.key_from_secret(b"edge forgeries: %x" % i)
        self.a, _ = S.expand_mini_secret(self.mini)
        self.point = E.pt_mul(self.a, E.BASE)
        self.pk = S.ristretto_encode(self.point)
        assert rist_class(self.pk) == "valid"
        self.outcome = key_sqrt_outcome(self.pk)

    def sign_as(self, pk_bytes: bytes, msg: bytes, r: int, R_bytes=None) -> bytes:
        """The signer's signature with `pk_bytes` in the transcript (and, given R_bytes, that R beside r)."""
        if R_bytes is None:
            R_bytes = S.ristretto_encode(E.pt_mul(r, E.BASE))
        k = S.challenge(pk_bytes, R_bytes, msg)
        return sr_sig(R_bytes, (k * self.a + r) % L)


def four_torsion():
    t = E.torsion_points()
    return [(x, y, 1, x * y % P) for (x, y) in t[::2]]


def coset_encodings(point):
    """Every 32-byte s < p with s^2 = (1 - y) / (1 + y) for a point (x, y) of
    the Ristretto coset point + E[4] that decodes into that coset once the two
    sign tests are left out (the others decode to the coset of -point), and
    the class of each."""
    out = {}
    for t4 in four_torsion():
        X, Y, Z, _ = E.pt_add(point, t4)
        y = Y * pow(Z, P - 2, P) % P
        if (1 + y) % P == 0:
            continue
        ok, s0 = S.sqrt_ratio_i((1 - y) % P, (1 + y) % P)
        if not ok:
            continue
        for s in {s0, (P - s0) % P}:
            pt, _ = rist_decode(b32(s), ("negative", "neg_t"))
            if pt is not None and S.ristretto_equal(pt, point):
                out[b32(s)] = rist_class(b32(s))
    return out


def rejected_encodings():
    """{class: [encodings]} of rejected Ristretto encodings, each failing its
    class's test first in the decoder's order."""
    cls, census = {}, {}
    for s in range(400):
        c = rist_class(b32(s))
        census[c[:9]] = census.get(c[:9], 0) + 1
        if c not in ("valid", "negative"):
            cls.setdefault(c, []).append(b32(s))
    # the 200 odd s are negative; the even ones split three ways
    assert census["negative"] == 200 and set(census) == {"negative", "nonsquare", "neg_t", "valid"}, census
    for c in ("nonsquare_flipped_i", "nonsquare_none"):
        assert len(cls[c]) >= 4, (c, len(cls.get(c, [])))
    out = {c: cls[c][:4] for c in ("nonsquare_flipped_i", "nonsquare_none")}
    out["neg_t"] = cls["neg_t"][:2]
    # negative: p - s of a valid s, so the sign test is the only one that fails,
    # and a plain small odd s
    valid_small = [b32(s) for s in range(2, 400, 2) if rist_class(b32(s)) == "valid"]
    neg = b32(P - int.from_bytes(valid_small[0], "little"))
    assert rist_decode(neg, "negative")[0] is not None
    out["negative"] = [neg, b32(3)]
    out["y_zero"] = [b32(P - 1)]
    # p and p + 18 are the ends of [p, 2^255); p + k with k itself a valid encoding fails on that test alone
    k_valid = next(k for k in range(2, 19, 2) if rist_class(b32(k)) == "valid")
    out["noncanonical"] = [b32(P), b32(P + 18), b32(P + k_valid)]
    over = b32(int.from_bytes(valid_small[1], "little") | 1 << 255)
    assert rist_decode(over, "bit255")[0] is not None
    out["bit255"] = [over]
    for c, encs in out.items():
        for e in encs:
            assert rist_class(e) == c, (c, e.hex(), rist_class(e))
    return out


def sr25519_records():
    rej = rejected_encodings()
    s_rand = rng.randrange(2, L - 1)
    scalars = [("0", 0), ("1", 1), ("rand", s_rand), ("l-1", L - 1)]

    # a rejected key that acts as the identity: R = [s]B verifies when key_ok is forgotten
    for c, encs in rej.items():
        for i, pk in enumerate(encs):
            for label, s in scalars:
                emit("sr25519", "key_identity/%s/%d/s=%s" % (c, i, label), "key_ok", pk, next_msg(), sr_base_sig(s), -1)

    # a rejected encoding of the signer's own point, in the transcript
    signers = [Signer(i) for i in range(8)]
    assert {sg.outcome for sg in signers} == {"correct", "flipped"}, [sg.outcome for sg in signers]
    for i, sg in enumerate(signers):
        alts = coset_encodings(sg.point)
        assert alts[sg.pk] == "valid" and list(alts.values()).count("valid") == 1
        assert list(alts.values()).count("neg_t") == 1 and list(alts.values()).count("negative") == 2, alts
        neg = b32(P - int.from_bytes(sg.pk, "little"))
        assert alts[neg] == "negative"
        negt = next(e for e, c in alts.items() if c == "neg_t")
        for enc, skip in ((neg, "negative"), (negt, "neg_t")):
            pt, _ = rist_decode(enc, skip)
            assert S.ristretto_equal(pt, sg.point), "the lax decoding leaves the signer's coset"
        over = b32(int.from_bytes(sg.pk, "little") | 1 << 255)
        for c, skip, enc in (("negative", "key_sign", neg), ("neg_t", "key_neg_t", negt),
                             ("bit255", "key_bit255", over)):
            if c == "bit255" and i >= 2:
                continue
            m = next_msg()
            emit("sr25519", "lax_key/%s/%d/%s" % (c, i, sg.outcome), skip, enc, m,
                 sg.sign_as(enc, m, rng.randrange(1, L)), -1)

    # a rejected R that acts as the identity, under the zero key with s = 0
    for c, encs in rej.items():
        for i, Rb in enumerate(encs[:2] if c == "noncanonical" else encs[:1]):
            emit("sr25519", "r_identity/%s/%d" % (c, i), "r_ok", ZERO32, next_msg(), sr_sig(Rb, 0), 0)

    # precedence: key, then scalar, then R
    bad = rej["nonsquare_none"][0]
    b = sr_base_sig(5)
    emit("sr25519", "precedence/bad_key_no_marker", "order_scalar_first", bad, next_msg(),
         sr_sig(b[:32], 5, marker=False), -1)
    emit("sr25519", "precedence/bad_key_s_eq_l", "order_scalar_first", bad, next_msg(), sr_sig(b[:32], L), -1)
    emit("sr25519", "precedence/s_eq_l_bad_r", "order_r_first", signers[0].pk, next_msg(),
         sr_sig(rej["neg_t"][0], L), -2)

    # scalar edges on honest signatures
    for i, sg in enumerate(signers[:2]):
        m = next_msg()
        sig = sg.sign_as(sg.pk, m, rng.randrange(1, L))
        assert sr_status(sg.pk, m, sig) == 1
        s = int.from_bytes(sig[32:], "little") & MASK255
        emit("sr25519", "scalar/s_plus_l/%d" % i, "s_lt_l", sg.pk, m, sr_sig(sig[:32], s + L), -2)
        emit("sr25519", "scalar/no_marker/%d" % i, "marker", sg.pk, m, sr_sig(sig[:32], s, marker=False), -2)

    # must accept
    for label, s in scalars + [("5", 5)]:
        emit("sr25519", "accept/zero_key/s=%s" % label, None, ZERO32, next_msg(), sr_base_sig(s), 1)
    picked = [next(sg for sg in signers if sg.outcome == o) for o in ("correct", "flipped")] + [signers[-1]]
    for i, sg in enumerate(picked):
        m = next_msg()
        emit("sr25519", "accept/r_identity/%d/%s" % (i, sg.outcome), None, sg.pk, m,
             sg.sign_as(sg.pk, m, 0, R_bytes=ZERO32), 1)
    for i, sg in enumerate(signers[2:4]):
        m = next_msg()
        emit("sr25519", "accept/honest/%d/%s" % (i, sg.outcome), None, sg.pk, m,
             sg.sign_as(sg.pk, m, rng.randrange(1, L)), 1)


# ---------------------------------------------------------------- ed25519

def ed_undecodable():
    """Encodings ZIP-215 decoding rejects (x^2 not a square): small y, found by
    search; one with the sign bit; y >= p, which the lax rules first reduce."""
    out = []
    y = 2
    while len(out) < 6:
        if E.recover_x(y, 0) is None:
            out.append(b32(y))
        y += 1
    out[5] = b32(int.from_bytes(out[5], "little") | 1 << 255)
    for k in range(19):
        if E.recover_x(k, 0) is None and len(out) < 8:
            out.append(b32(P + k))
    y = 1 << 254
    while len(out) < 8:
        if E.recover_x(y % P, 0) is None:
            out.append(b32(y))
        y += 1
    for e in out:
        assert E.decode_point_zip215(e) is None
    return out


class EdSigner:
    def __init__(self, i: int):
        self.seed = hashlib.sha256(b"edge forgeries ed: %x" % i).digest()
        self.a, self.prefix = E.expand_seed(self.seed)
        self.point = E.pt_mul(self.a, E.BASE)
        self.pk = E.pt_encode(self.point)


def ed25519_records():
    undec = ed_undecodable()
    s_rand = rng.randrange(2, L - 1)
    scalars = [("0", 0), ("1", 1), ("rand", s_rand), ("l-1", L - 1)]

    for i, A in enumerate(undec):
        for label, s in scalars:
            emit("ed25519", "a_identity/%d/S=%s" % (i, label), "a_decode", A, next_msg(),
                 E.pt_encode(E.pt_mul(s, E.BASE)) + b32(s), 0)

    small = E.small_order_encodings()
    assert len(small) == 14
    for j, A in enumerate(small):
        for i in range(4):
            emit("ed25519", "r_identity/A%d/%d" % (j, i), "r_decode", A, next_msg(),
                 undec[(j + 2 * i) % len(undec)] + ZERO32, 0)

    signers = [EdSigner(i) for i in range(2)]
    for i, sg in enumerate(signers):
        m = next_msg()
        sig = E.sign(sg.seed, m)
        assert ed_status(sg.pk, m, sig) == 1
        Sv = int.from_bytes(sig[32:], "little")
        for label, mult in (("s_plus_l", 1), ("s_plus_2l", 2)):
            assert Sv + mult * L < 1 << 256
            emit("ed25519", "scalar/%s/%d" % (label, i), "s_lt_l", sg.pk, m, sig[:32] + b32(Sv + mult * L), 0)

    # mixed order: a prime-order point plus a torsion point, as R, as A, as both
    torsion = [(x, y, 1, x * y % P) for (x, y) in E.torsion_points()]
    assert len(torsion) == 8
    for t, T in enumerate(torsion):
        order = next(o for o in (1, 2, 4, 8) if E.pt_is_identity(E.pt_mul(o, T)))
        for i, sg in enumerate(signers):
            for shape in ("mixed_r", "mixed_a", "mixed_both"):
                m = next_msg()
                r = rng.randrange(1, L)
                R = E.pt_mul(r, E.BASE)
                Rb = E.pt_encode(E.pt_add(R, T) if shape != "mixed_a" else R)
                Ab = E.pt_encode(E.pt_add(sg.point, T)) if shape != "mixed_r" else sg.pk
                k = E.sha512_modl(Rb, Ab, m)
                emit("ed25519", "accept/%s/T%d_order%d/%d" % (shape, t, order, i), None, Ab, m,
                     Rb + b32((r + k * sg.a) % L), 1)


def render() -> str:
    """The fixture's text, built afresh (every assertion above runs)."""
    records.clear()
    rng.seed(SEED)
    sr25519_records()
    ed25519_records()
    doc = {"source": "tests/golden/make_edge_forgeries_golden.py; verdicts from oracle/ed25519_ref.py (ZIP-215) and "
                     "oracle/sr25519_ref.py (the restatement's own: the reference holds no vector for these, and the "
                     "zero sr25519 key accepted as valid is the restatement's reading; parity with voi unpinned)",
           "vectors": records}
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


def main():
    text = render()
    with open(os.path.join(HERE, "edge_forgeries.json"), "w") as f:
        f.write(text)
    tags = {}
    for r in records:
        key = (r["scheme"], r["skipped_check"], r["status"])
        tags[key] = tags.get(key, 0) + 1
    for key in sorted(tags, key=str):
        print("%-8s %-20s status %2d: %d" % (*key, tags[key]))
    print(len(records), "records written")


if __name__ == "__main__":
    main()
