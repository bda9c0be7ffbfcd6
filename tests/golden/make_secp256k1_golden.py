"""Writes tests/golden/secp256k1_vectors.json: the smallest inputs at which a
secp256k1 ECDSA verifier can go wrong.  Every verdict is computed by the
big-integer restatement tests/secp256k1_ref.py; OpenSSL's ECDSA_do_verify,
with the reference's rules 3-4 (lower-S, ranges) and the compressed-key rule
applied beside it, must agree on every vector, and the families whose verdict
is known by construction assert it.

Parity with btcec itself is unpinned by reference-held vectors: nothing here
can run it.  The families restate the reference's own tests
(crypto/secp256k1/secp256k1_test.go: TestSignAndValidateSecp256k1,
TestSignatureVerificationAndRejectUpperS, TestGenPrivKeySecp256k1).

    python tests/golden/make_secp256k1_golden.py
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import secp256k1_ref as R  # noqa: E402
from tendermint_amd.testing import secp256k1_factory as F  # noqa: E402

N, P = R.N, R.P
HALF = N >> 1
vectors = []


def sha(m: bytes) -> bytes:
    return hashlib.sha256(m).digest()


def zint(m: bytes) -> int:
    return int.from_bytes(sha(m), "big")


def b32(x: int) -> bytes:
    return x.to_bytes(32, "big")


def emit(name: str, pk: bytes, msg: bytes, sig: bytes, want=None):
    v = R.verify(pk, msg, sig)
    if want is not None:
        assert v == want, (name, v, want)
    if F.have_openssl():
        assert F.openssl_verdict(pk, sha(msg), sig) == v, ("OpenSSL disagrees", name, v)
    vectors.append({"name": name, "pk": pk.hex(), "msg": msg.hex(), "sig": sig.hex(), "valid": v})


def flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def crafted_key(msg: bytes, k: int, s: int):
    """(pk, sig) with the chosen nonce k and s: d = (s k - z) / r."""
    r = F.mul_g(k)[0] % N
    d = (s * k - zint(msg)) * pow(r, -1, N) % N
    assert d != 0
    return F.compress(F.mul_g(d)), b32(r) + b32(s)


BATCH_N, BATCH_SEED = 4096, 0x5EC9


def batch_verdicts():
    """tests/golden/secp256k1_batch4096.json: the restatement's verdicts of the
    generated 4,096-entry batch (make_secp_batch, about 5% corrupted), each
    cross-checked with OpenSSL, pinned to the batch's bytes by a digest; the
    device test's smaller batches are prefixes of it."""
    from collections import Counter
    b = F.make_secp_batch(BATCH_N, seed=BATCH_SEED)
    counts = Counter(b.entry(i)[0] for i in range(b.n))
    combs = {pk: R.comb_table(R.parse_pubkey(pk)) for pk, k in counts.items() if k >= 16}
    keys = {}
    valid = []
    for i in range(b.n):
        pk, msg, sig = b.entry(i)
        v = R.verify(pk, msg, sig, combs=combs)
        assert v == (b.category[i] == "honest"), (i, b.category[i], v)
        if F.have_openssl():
            assert F.openssl_verdict(pk, sha(msg), sig) == v, ("OpenSSL disagrees", i, b.category[i])
        valid.append(v)
    bits = bytearray((b.n + 7) // 8)
    for i, v in enumerate(valid):
        bits[i >> 3] |= int(v) << (i & 7)
    with open(os.path.join(HERE, "secp256k1_batch4096.json"), "w") as f:
        json.dump({"n": b.n, "seed": BATCH_SEED, "sha256": F.batch_digest(b), "valid_bits": bits.hex(),
                   "categories": dict(Counter(b.category))}, f, indent=1)
        f.write("\n")
    print(f"batch of {b.n}: {sum(valid)} valid, categories {dict(Counter(b.category))}")


def main():
    rng = random.Random(0x5EC9256)
    # A. honest signatures of GenPrivKeySecp256k1 keys, each with one flipped bit
    for i in range(8):
        s = F.Secp256k1Signer.from_secret(f"key: {i:x}".encode())
        msg = b"secp256k1 vote %d" % i
        sig = s.sign(msg)
        emit(f"honest/{i}", s.public_key, msg, sig, True)
        emit(f"honest/{i}/flip_r", s.public_key, msg, flip(sig, rng.randrange(256)), False)
        emit(f"honest/{i}/flip_s", s.public_key, msg, flip(sig, 256 + rng.randrange(256)), False)
        emit(f"honest/{i}/flip_msg", s.public_key, flip(msg, rng.randrange(8 * len(msg))), sig, False)
        emit(f"honest/{i}/flip_key", flip(s.public_key, 8 + rng.randrange(256)), msg, sig, False)
    # B. TestSignatureVerificationAndRejectUpperS
    for i in range(4):
        s = F.Secp256k1Signer.from_secret(b"upper-s %d" % i)
        msg = b"We have lingered long enough on the shores of the cosmic ocean."
        sig = s.sign(msg)
        emit(f"upper_s/{i}/low", s.public_key, msg, sig, True)
        emit(f"upper_s/{i}/negated", s.public_key, msg, sig[:32] + b32(N - int.from_bytes(sig[32:], "big")), False)
    for name, sv, want in (("half", HALF, True), ("half_plus_1", HALF + 1, False), ("one", 1, True)):
        for i in range(2):
            msg = b"crafted s %s %d" % (name.encode(), i)
            pk, sig = crafted_key(msg, rng.randrange(1, N), sv)
            emit(f"s_edge/{name}/{i}", pk, msg, sig, want)
    # C. range edges
    s = F.Secp256k1Signer.from_secret(b"range")
    msg = b"range edges"
    sig = s.sign(msg)
    rr, ss = sig[:32], sig[32:]
    for name, r_, s_ in (("r_zero", bytes(32), ss), ("s_zero", rr, bytes(32)), ("r_n", b32(N), ss),
                         ("r_n_minus_1", b32(N - 1), ss), ("r_n_plus_5", b32(N + 5), ss),
                         ("r_plus_n", b32(int.from_bytes(rr, "big") + N) if int.from_bytes(rr, "big") + N < 2**256
                          else b32(N + 1), ss),
                         ("r_max", b"\xff" * 32, ss), ("s_max", rr, b"\xff" * 32), ("s_n", rr, b32(N)),
                         ("s_n_minus_1", rr, b32(N - 1)), ("both_zero", bytes(32), bytes(32))):
        emit(f"range/{name}", s.public_key, msg, r_ + s_, False)
    # D. key edges
    for pre in (0x00, 0x04, 0x05, 0x06, 0x07):
        emit(f"key/prefix_{pre:02x}", bytes([pre]) + s.public_key[1:], msg, sig, False)
    for name, x in (("x_p", P), ("x_p_plus_1", P + 1), ("x_max", 2**256 - 1), ("x_no_root", F.non_residue_x(rng))):
        for pre in (2, 3):
            emit(f"key/{name}/{pre}", bytes([pre]) + b32(x), msg, sig, False)
    emit("key/other_parity", bytes([s.public_key[0] ^ 1]) + s.public_key[1:], msg, sig, False)
    # x = 0 is off the curve (7 is not a square mod p)
    emit("key/x_zero", b"\x02" + bytes(32), msg, sig, False)
    # E. exceptional group cases: Q = +-G, +-2G, 3G meets the G windows
    for d in (1, 2, 3, N - 1, N - 2):
        signer = F.Secp256k1Signer(d)
        dn = {1: "1", 2: "2", 3: "3", N - 1: "n-1", N - 2: "n-2"}[d]
        for i in range(64):
            m = b"q=%sG #%d" % (dn.encode(), i)
            emit(f"small_key/{dn}/{i}", signer.public_key, m, signer.sign(m), True)
    # F. forgeries that drive R' to infinity: r = -z / d
    for dn, d in (("1", 1), ("2", 2), ("3", 3), ("n-1", N - 1), ("gen", F.gen_priv_key_secp256k1(b"inf"))):
        pk = F.compress(F.mul_g(d))
        for i in range(2):
            m = b"to infinity %d" % i
            r = -zint(m) * pow(d, -1, N) % N
            emit(f"infinity/{dn}/{i}", pk, m, b32(r) + b32(rng.randrange(1, HALF)), False)
    # G. u1 = +-u2: r = +-z mod n
    for d in (1, 2, 3, N - 1, N - 2):
        pk = F.compress(F.mul_g(d))
        dn = {1: "1", 2: "2", 3: "3", N - 1: "n-1", N - 2: "n-2"}[d]
        for sign in (1, -1):
            m = b"u1 = %su2 under %s" % (b"" if sign > 0 else b"-", dn.encode())
            emit(f"u1_eq_u2/{dn}/{'plus' if sign > 0 else 'minus'}", pk, m,
                 b32(sign * zint(m) % N) + b32(rng.randrange(1, HALF)))
    # H. x(R') >= n: the reference reduces x mod n, so r = x - n verifies
    # (x = n is itself on the curve, but r = 0 is out of range: the first x after it)
    x = N + 1
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) != 1:
        x += 1
    assert N < x < P
    y = pow((x ** 3 + 7) % P, (P + 1) // 4, P)
    for i, yy in enumerate((y, P - y)):
        Rpt = (x, yy)
        r = x - N
        sv = rng.randrange(1, HALF)
        m = b"x(R) >= n %d" % i
        # Q = (s R - z G) / r
        sR = R.mul(sv, Rpt)
        zG = R.mul(zint(m), R.G)
        Q = R.mul(pow(r, -1, N), R.add_affine(sR, R.neg_affine(zG)))
        emit(f"x_ge_n/{i}", R.compress(Q), m, b32(r) + b32(sv), True)
        emit(f"x_ge_n/{i}/r_off_by_one", R.compress(Q), m, b32(r + 1) + b32(sv), False)
    # I. message lengths at SHA-256 block edges
    s = F.Secp256k1Signer.from_secret(b"lengths")
    for ln in (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000):
        m = bytes(rng.randrange(256) for _ in range(ln))
        emit(f"msg_len/{ln}", s.public_key, m, s.sign(m), True)
    out = os.path.join(HERE, "secp256k1_vectors.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(v, separators=(",", ":")) for v in vectors) + "\n]\n")
    batch_verdicts()
    n_valid = sum(v["valid"] for v in vectors)
    print(f"{len(vectors)} vectors ({n_valid} valid), {os.path.getsize(out)} bytes, "
          f"OpenSSL cross-check: {'yes' if F.have_openssl() else 'NOT AVAILABLE'}")


if __name__ == "__main__":
    main()
