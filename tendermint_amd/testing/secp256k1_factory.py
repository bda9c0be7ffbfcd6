"""secp256k1 keys, signatures and synthetic batches for tests and tools.

Keys follow the reference's GenPrivKeySecp256k1 (crypto/secp256k1/
secp256k1.go:112-129: d = SHA-256(secret) mod (n - 1) + 1); signatures are
deterministic RFC 6979 (HMAC-SHA-256) ECDSA over SHA-256(msg), normalised to
lower-S, serialised r || s (secp256k1.go:192-204).  Input generation only:
the tests take their expected verdicts from tests/secp256k1_ref.py.

OpenSSL's libcrypto (ctypes) is used where present for fast signing
(OpensslKey.sign, the nonce's point in sign_digest) and as a second ECDSA
verifier (OpensslKey.verify).  It does not
enforce lower-S or the range rules' exact form, so callers apply those beside
it (openssl_verdict).
"""
from __future__ import annotations

import ctypes
import ctypes.util
import hashlib
import hmac
import random
from dataclasses import dataclass, field
from typing import List

import numpy as np

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8


# ---------------------------------------------------------------- curve (signing side)
def _jdbl(a):
    X, Y, Z = a
    if Z == 0:
        return a
    A, B = X * X % P, Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) ** 2 - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return (X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P)


def _jadd_affine(a, b):
    """a (Jacobian) + b (affine); b is never a's equal or negative here except by the checks below."""
    X1, Y1, Z1 = a
    if Z1 == 0:
        return (b[0], b[1], 1)
    ZZ = Z1 * Z1 % P
    U2, S2 = b[0] * ZZ % P, b[1] * Z1 * ZZ % P
    if U2 == X1:
        return _jdbl(a) if S2 == Y1 else (1, 1, 0)
    H, R = U2 - X1, S2 - Y1
    HH = H * H % P
    HHH, V = H * HH % P, X1 * HH % P
    X3 = (R * R - HHH - 2 * V) % P
    return (X3, (R * (V - X3) - Y1 * HHH) % P, Z1 * H % P)


def _affine(a):
    if a[2] == 0:
        return None
    zi = pow(a[2], -1, P)
    return (a[0] * zi * zi % P, a[1] * zi * zi * zi % P)


_POW2_G: list = []


def mul_g(k: int):
    """k G (affine, None for infinity) over a table of 2^i G."""
    if not _POW2_G:
        pt = (GX, GY)
        for _ in range(256):
            _POW2_G.append(pt)
            pt = _affine(_jdbl((pt[0], pt[1], 1)))
    acc = (1, 1, 0)
    k %= N
    i = 0
    while k:
        if k & 1:
            acc = _jadd_affine(acc, _POW2_G[i])
        k >>= 1
        i += 1
    return _affine(acc)


def compress(pt) -> bytes:
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


# ---------------------------------------------------------------- keys and signing
def gen_priv_key_secp256k1(secret: bytes) -> int:
    """GenPrivKeySecp256k1 (secp256k1.go:112-129)."""
    return int.from_bytes(hashlib.sha256(secret).digest(), "big") % (N - 1) + 1


def rfc6979_k(d: int, z32: bytes) -> int:
    """RFC 6979 section 3.2 nonce for HMAC-SHA-256, qlen = 256."""
    x = d.to_bytes(32, "big")
    h1 = (int.from_bytes(z32, "big") % N).to_bytes(32, "big")
    V, K = b"\x01" * 32, b"\x00" * 32
    K = hmac.new(K, V + b"\x00" + x + h1, hashlib.sha256).digest()
    V = hmac.new(K, V, hashlib.sha256).digest()
    K = hmac.new(K, V + b"\x01" + x + h1, hashlib.sha256).digest()
    V = hmac.new(K, V, hashlib.sha256).digest()
    while True:
        V = hmac.new(K, V, hashlib.sha256).digest()
        k = int.from_bytes(V, "big")
        if 1 <= k < N:
            return k
        K = hmac.new(K, V + b"\x00", hashlib.sha256).digest()
        V = hmac.new(K, V, hashlib.sha256).digest()


def sign_digest(d: int, z32: bytes, k: int | None = None) -> bytes:
    """ECDSA over a 32-byte digest, lower-S, r || s.  k: nonce override (tests)."""
    z = int.from_bytes(z32, "big")
    bump = 0
    while True:
        kk = k if k is not None else rfc6979_k(d, hashlib.sha256(z32 + bytes([bump])).digest() if bump else z32)
        r = _mul_g_x(kk) % N
        s = pow(kk, -1, N) * (z + r * d) % N
        if r and s:
            break
        if k is not None:
            raise ValueError("nonce gives r = 0 or s = 0")
        bump += 1
    if s > N >> 1:
        s = N - s
    return r.to_bytes(32, "big") + s.to_bytes(32, "big")


class Secp256k1Signer:
    def __init__(self, d: int):
        assert 1 <= d < N
        self.d = d
        self.public_key = compress(mul_g(d))

    @classmethod
    def from_secret(cls, secret: bytes) -> "Secp256k1Signer":
        return cls(gen_priv_key_secp256k1(secret))

    def sign(self, msg: bytes) -> bytes:
        return sign_digest(self.d, hashlib.sha256(msg).digest())


# ---------------------------------------------------------------- OpenSSL (optional)
_NID_SECP256K1 = 714
_ssl = None


def _openssl():
    global _ssl
    if _ssl is None:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp = ctypes.c_void_p
        L.EC_KEY_new_by_curve_name.restype = vp
        L.EC_KEY_new_by_curve_name.argtypes = [ctypes.c_int]
        L.EC_KEY_free.argtypes = [vp]
        L.EC_KEY_get0_group.restype = vp
        L.EC_KEY_get0_group.argtypes = [vp]
        L.EC_POINT_new.restype = vp
        L.EC_POINT_new.argtypes = [vp]
        L.EC_POINT_free.argtypes = [vp]
        L.EC_POINT_oct2point.argtypes = [vp, vp, ctypes.c_char_p, ctypes.c_size_t, vp]
        L.EC_KEY_set_public_key.argtypes = [vp, vp]
        L.EC_KEY_set_private_key.argtypes = [vp, vp]
        L.BN_bin2bn.restype = vp
        L.BN_bin2bn.argtypes = [ctypes.c_char_p, ctypes.c_int, vp]
        L.BN_bn2binpad.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
        L.BN_free.argtypes = [vp]
        L.ECDSA_SIG_new.restype = vp
        L.ECDSA_SIG_free.argtypes = [vp]
        L.ECDSA_SIG_set0.argtypes = [vp, vp, vp]
        L.ECDSA_SIG_get0_r.restype = vp
        L.ECDSA_SIG_get0_r.argtypes = [vp]
        L.ECDSA_SIG_get0_s.restype = vp
        L.ECDSA_SIG_get0_s.argtypes = [vp]
        L.ECDSA_do_verify.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, vp]
        L.ECDSA_do_sign.restype = vp
        L.ECDSA_do_sign.argtypes = [ctypes.c_char_p, ctypes.c_int, vp]
        L.ERR_clear_error.argtypes = []
        if not L.EC_KEY_new_by_curve_name(_NID_SECP256K1):
            raise RuntimeError("libcrypto has no secp256k1")
        _ssl = L
    return _ssl


def have_openssl() -> bool:
    try:
        _openssl()
        return True
    except Exception:
        return False


class OpensslKey:
    """An EC_KEY for a compressed public key (None when OpenSSL rejects the encoding)."""

    def __init__(self, pk: bytes, d: int | None = None):
        L = _openssl()
        self._L = L
        self.key = L.EC_KEY_new_by_curve_name(_NID_SECP256K1)
        grp = L.EC_KEY_get0_group(self.key)
        pt = L.EC_POINT_new(grp)
        self.ok = L.EC_POINT_oct2point(grp, pt, pk, len(pk), None) == 1 and L.EC_KEY_set_public_key(self.key, pt) == 1
        L.EC_POINT_free(pt)
        if d is not None:
            bn = L.BN_bin2bn(d.to_bytes(32, "big"), 32, None)
            L.EC_KEY_set_private_key(self.key, bn)
            L.BN_free(bn)
        L.ERR_clear_error()

    def verify(self, z32: bytes, sig: bytes) -> bool:
        """Plain ECDSA (no lower-S rule): ECDSA_do_verify == 1."""
        if not self.ok:
            return False
        L = self._L
        s = L.ECDSA_SIG_new()
        L.ECDSA_SIG_set0(s, L.BN_bin2bn(sig[:32], 32, None), L.BN_bin2bn(sig[32:], 32, None))
        rc = L.ECDSA_do_verify(z32, 32, s, self.key)
        L.ECDSA_SIG_free(s)
        L.ERR_clear_error()
        return rc == 1

    def sign(self, z32: bytes) -> bytes:
        """Randomised ECDSA from libcrypto, normalised to lower-S (bulk inputs for benchmarks)."""
        L = self._L
        s = L.ECDSA_do_sign(z32, 32, self.key)
        rb, sb = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        L.BN_bn2binpad(L.ECDSA_SIG_get0_r(s), rb, 32)
        L.BN_bn2binpad(L.ECDSA_SIG_get0_s(s), sb, 32)
        L.ECDSA_SIG_free(s)
        sv = int.from_bytes(sb.raw, "big")
        if sv > N >> 1:
            sv = N - sv
        return rb.raw + sv.to_bytes(32, "big")

    def __del__(self):
        try:
            self._L.EC_KEY_free(self.key)
        except Exception:
            pass


def _mul_g_x(k: int) -> int:
    """x(k G): through libcrypto where present (the bulk signer's one curve
    operation), else the table above.  The same value either way."""
    if not have_openssl():
        return mul_g(k)[0]
    L = _openssl()
    if not hasattr(L, "_secp_group"):
        vp = ctypes.c_void_p
        L.EC_GROUP_new_by_curve_name.restype = vp
        L.EC_GROUP_new_by_curve_name.argtypes = [ctypes.c_int]
        L.EC_POINT_mul.argtypes = [vp] * 6
        L.EC_POINT_get_affine_coordinates.argtypes = [vp] * 5
        L.BN_new.restype = vp
        L._secp_group = L.EC_GROUP_new_by_curve_name(_NID_SECP256K1)
        L._secp_pt = L.EC_POINT_new(L._secp_group)
        L._secp_x = L.BN_new()
    kb = L.BN_bin2bn(k.to_bytes(32, "big"), 32, None)
    ok = L.EC_POINT_mul(L._secp_group, L._secp_pt, kb, None, None, None) == 1 and \
        L.EC_POINT_get_affine_coordinates(L._secp_group, L._secp_pt, L._secp_x, None, None) == 1
    L.BN_free(kb)
    if not ok:
        L.ERR_clear_error()
        return mul_g(k)[0]
    out = ctypes.create_string_buffer(32)
    L.BN_bn2binpad(L._secp_x, out, 32)
    return int.from_bytes(out.raw, "big")


def openssl_verdict(pk: bytes, z32: bytes, sig: bytes) -> bool:
    """OpenSSL's ECDSA verdict with the reference's rules 3-4 applied beside it
    (lower-S; 1 <= r, s < n) and the compressed-only key rule."""
    if len(pk) != 33 or pk[0] not in (2, 3) or len(sig) != 64:
        return False
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if not (1 <= r < N and 1 <= s < N) or s > N >> 1:
        return False
    return OpensslKey(pk).verify(z32, sig)


# ---------------------------------------------------------------- batches
@dataclass
class SecpBatch:
    pk: np.ndarray    # n*33 uint8
    sig: np.ndarray   # n*64 uint8
    msg: np.ndarray   # concatenated uint8
    off: np.ndarray   # n+1 uint32
    n: int
    category: List[str] = field(default_factory=list)  # "honest" or the corruption applied

    def entry(self, i: int):
        return (self.pk[33 * i:33 * i + 33].tobytes(), self.msg[self.off[i]:self.off[i + 1]].tobytes(),
                self.sig[64 * i:64 * i + 64].tobytes())

    def prefix(self, n: int) -> "SecpBatch":
        return SecpBatch(self.pk[:33 * n].copy(), self.sig[:64 * n].copy(), self.msg[:self.off[n]].copy(),
                         self.off[:n + 1].copy(), n, self.category[:n])


def non_residue_x(rng: random.Random) -> int:
    while True:
        x = rng.randrange(P)
        c = (x * x * x + 7) % P
        if pow(c, (P - 1) // 2, P) != 1:
            return x


CORRUPTIONS = ["flip_r", "flip_s", "flip_msg", "flip_key", "upper_s", "r_zero", "s_zero", "r_ge_n", "s_max",
               "prefix", "x_ge_p", "x_no_root", "parity"]


def corrupt(kind: str, pk: bytes, msg: bytes, sig: bytes, rng: random.Random):
    pk, msg, sig = bytearray(pk), bytearray(msg), bytearray(sig)
    if kind == "flip_r":
        sig[rng.randrange(32)] ^= 1 << rng.randrange(8)
    elif kind == "flip_s":
        sig[32 + rng.randrange(32)] ^= 1 << rng.randrange(8)
    elif kind == "flip_msg":
        if msg:
            msg[rng.randrange(len(msg))] ^= 1 << rng.randrange(8)
        else:
            msg = bytearray(b"\x01")
    elif kind == "flip_key":
        pk[1 + rng.randrange(32)] ^= 1 << rng.randrange(8)
    elif kind == "upper_s":
        sig[32:] = (N - int.from_bytes(sig[32:], "big")).to_bytes(32, "big")
    elif kind == "r_zero":
        sig[:32] = bytes(32)
    elif kind == "s_zero":
        sig[32:] = bytes(32)
    elif kind == "r_ge_n":
        sig[:32] = (N + rng.randrange(1 << 64)).to_bytes(32, "big")
    elif kind == "s_max":
        sig[32:] = b"\xff" * 32
    elif kind == "prefix":
        pk[0] = rng.choice([0x00, 0x04, 0x05, 0x06])
    elif kind == "x_ge_p":
        pk[1:] = (P + rng.randrange(2**32 + 977)).to_bytes(32, "big")
    elif kind == "x_no_root":
        pk[1:] = non_residue_x(rng).to_bytes(32, "big")
    elif kind == "parity":
        pk[0] ^= 1
    else:
        raise ValueError(kind)
    return bytes(pk), bytes(msg), bytes(sig)


def batch_digest(b: "SecpBatch") -> str:
    """SHA-256 over the batch's bytes (pins a generated batch to stored verdicts)."""
    return hashlib.sha256(b.pk.tobytes() + b.sig.tobytes() + b.msg.tobytes() + b.off.tobytes()).hexdigest()


def make_secp_batch(n: int, seed: int = 0x5EC9, bad_frac: float = 0.05, keys: int = 32, bad_at=(),
                    msg_lens=None, fast: bool = False) -> SecpBatch:
    """n signatures over commit-vote-like messages by `keys` validators, with
    about bad_frac of the entries corrupted (round-robin over CORRUPTIONS) and
    the entries listed in bad_at corrupted by a key-parse failure.  msg_lens:
    explicit message lengths.  fast: sign through libcrypto (random nonces; the
    batch is then not reproducible byte for byte)."""
    from ..types.canonical import BlockID, PartSetHeader, Timestamp, vote_sign_bytes, PRECOMMIT_TYPE
    rng = random.Random(seed)
    signers = [Secp256k1Signer.from_secret(f"key: {i:x}".encode()) for i in range(min(keys, max(n, 1)))]
    ossl = [OpensslKey(s.public_key, s.d) for s in signers] if fast else None
    bid = BlockID(hashlib.sha256(b"block").digest(), PartSetHeader(1, hashlib.sha256(b"parts").digest()))
    pks, sigs, msgs, cats = [], [], [], []
    n_bad = 0
    for i in range(n):
        k = i % len(signers)
        if msg_lens is not None:
            msg = bytes(rng.randrange(256) for _ in range(msg_lens[i]))
        else:
            msg = vote_sign_bytes("secp-chain", PRECOMMIT_TYPE, 1 + i // len(signers), 0, bid,
                                  Timestamp(1577836800 + i, rng.randrange(10**9)))
        z = hashlib.sha256(msg).digest()
        sig = ossl[k].sign(z) if fast else sign_digest(signers[k].d, z)
        pk, cat = signers[k].public_key, "honest"
        if i in bad_at:
            cat = ("prefix", "x_no_root", "x_ge_p")[len(cats) % 3]
        elif rng.random() < bad_frac:
            cat = CORRUPTIONS[n_bad % len(CORRUPTIONS)]
            n_bad += 1
        if cat != "honest":
            pk, msg, sig = corrupt(cat, pk, msg, sig, rng)
        pks.append(pk)
        sigs.append(sig)
        msgs.append(msg)
        cats.append(cat)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return SecpBatch(np.frombuffer(b"".join(pks), dtype=np.uint8).copy(),
                     np.frombuffer(b"".join(sigs), dtype=np.uint8).copy(),
                     np.frombuffer(b"".join(msgs), dtype=np.uint8).copy(), off, n, cats)
