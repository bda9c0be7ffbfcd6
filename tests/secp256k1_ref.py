"""Big-integer restatement of secp256k1 PubKey.VerifySignature
(crypto/secp256k1/secp256k1.go:206-226 over btcec v0.22.1 ParsePubKey and
Go's ecdsa.Verify) -- the oracle of the secp256k1 tests.  Independent of the
product's arithmetic: Python integers, Jacobian coordinates with explicit
case analysis, a fixed-base table for G and 4-bit windows for Q.

verify(pk, msg, sig) is true only if
  1. len(sig) == 64, r = BE(sig[:32]), s = BE(sig[32:])
  2. the key parses: 33 bytes, prefix 0x02 / 0x03, x < p, y = (x^3+7)^((p+1)/4)
     with y^2 == x^3 + 7, y negated to the prefix's parity
  3. s <= n >> 1
  4. 1 <= r < n and 1 <= s < n
  5. z = BE(SHA-256(msg)), all 256 bits
  6. w = 1/s, u1 = z w, u2 = r w (mod n), R' = u1 G + u2 Q
  7. R' is not infinity
  8. x(R') mod n == r
"""
import hashlib

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
INF = None  # affine infinity; Jacobian infinity is Z == 0


def on_curve(pt) -> bool:
    return pt is INF or (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def jdouble(a):
    X, Y, Z = a
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    A = X * X % P
    B = Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) ** 2 - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return (X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P)


def jadd(a, b):
    X1, Y1, Z1 = a
    X2, Y2, Z2 = b
    if Z1 == 0:
        return b
    if Z2 == 0:
        return a
    Z1Z1 = Z1 * Z1 % P
    Z2Z2 = Z2 * Z2 % P
    U1 = X1 * Z2Z2 % P
    U2 = X2 * Z1Z1 % P
    S1 = Y1 * Z2 * Z2Z2 % P
    S2 = Y2 * Z1 * Z1Z1 % P
    if U1 == U2:
        return jdouble(a) if S1 == S2 else (1, 1, 0)
    H = U2 - U1
    R = S2 - S1
    HH = H * H % P
    HHH = H * HH % P
    V = U1 * HH % P
    X3 = (R * R - HHH - 2 * V) % P
    return (X3, (R * (V - X3) - S1 * HHH) % P, Z1 * Z2 * H % P)


def to_jacobian(pt):
    return (1, 1, 0) if pt is INF else (pt[0], pt[1], 1)


def to_affine(a):
    X, Y, Z = a
    if Z == 0:
        return INF
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def add_affine(p1, p2):
    return to_affine(jadd(to_jacobian(p1), to_jacobian(p2)))


def neg_affine(pt):
    return INF if pt is INF else (pt[0], (-pt[1]) % P)


def _window_table(pt):
    """[0, pt, 2pt, ..., 15pt] in Jacobian form."""
    tab = [(1, 1, 0), to_jacobian(pt)]
    for _ in range(14):
        tab.append(jadd(tab[-1], tab[1]))
    return tab


_G_COMB = None


def comb_table(pt):
    """table[i][d] = d 16^i pt (Jacobian with Z = 1 where finite): a scalar
    multiple of pt is then at most 64 additions and no doubling."""
    rows, base = [], pt
    for _ in range(64):
        rows.append([to_jacobian(a) for a in (to_affine(t) for t in _window_table(base))])
        base = to_affine(jdouble(jdouble(jdouble(jdouble(to_jacobian(base))))))
    return rows


def mul_comb_jacobian(k: int, comb):
    k %= N
    acc = (1, 1, 0)
    i = 0
    while k:
        d = k & 15
        if d:
            acc = jadd(acc, comb[i][d])
        k >>= 4
        i += 1
    return acc


def mul_g_jacobian(k: int):
    global _G_COMB
    if _G_COMB is None:
        _G_COMB = comb_table(G)
    return mul_comb_jacobian(k, _G_COMB)


def mul_jacobian(k: int, pt):
    k %= N
    tab = _window_table(pt)
    acc = (1, 1, 0)
    for i in range(63, -1, -1):
        acc = jdouble(jdouble(jdouble(jdouble(acc))))
        d = (k >> (4 * i)) & 15
        if d:
            acc = jadd(acc, tab[d])
    return acc


def mul(k: int, pt):
    return to_affine(mul_g_jacobian(k) if pt == G else mul_jacobian(k, pt))


def compress(pt) -> bytes:
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def parse_pubkey(pk: bytes):
    """btcec ParsePubKey, compressed form only; None when it does not parse."""
    if len(pk) != 33 or pk[0] not in (2, 3):
        return None
    x = int.from_bytes(pk[1:], "big")
    if x >= P:
        return None
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    if (y & 1) != (pk[0] & 1):
        y = P - y
    return (x, y)


def verify_digest(pk: bytes, z32: bytes, sig: bytes, combs=None) -> bool:
    """combs: optional {public key bytes: comb_table(its point)} for keys that
    verify many signatures (same arithmetic, fewer operations)."""
    if len(sig) != 64:
        return False
    r = int.from_bytes(sig[:32], "big")
    s = int.from_bytes(sig[32:], "big")
    q = parse_pubkey(pk)
    if q is None:
        return False
    if s > N >> 1:
        return False
    if not (1 <= r < N and 1 <= s < N):
        return False
    z = int.from_bytes(z32, "big")
    w = pow(s, -1, N)
    u1 = z * w % N
    u2 = r * w % N
    u2q = mul_comb_jacobian(u2, combs[pk]) if combs is not None and pk in combs else mul_jacobian(u2, q)
    rp = to_affine(jadd(mul_g_jacobian(u1), u2q))
    if rp is INF:
        return False
    return rp[0] % N == r


def verify(pk: bytes, msg: bytes, sig: bytes, combs=None) -> bool:
    return verify_digest(pk, hashlib.sha256(msg).digest(), sig, combs)
