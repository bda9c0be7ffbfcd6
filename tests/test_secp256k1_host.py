"""tendermint_amd/csrc/secp256k1.h compiled for the host with limb-bound
assertions (tests/native/secp), against Python integers and the big-integer
restatement tests/secp256k1_ref.py.  No GPU."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import secp256k1_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libsecpcheck.so")
P, N = R.P, R.N
ALL_ONES_LIMBS = sum(0x3FFFFFF << (26 * i) for i in range(9)) | (0x3FFFFF << 234)  # 2^256 - 1


@pytest.fixture(scope="module")
def S():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "secp")], check=True)
    L = ctypes.CDLL(SO)
    L.secpcheck_verify_msg.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.c_char_p, ctypes.c_size_t]
    return L


def b32(x):
    return x.to_bytes(32, "big")


def out32():
    return ctypes.create_string_buffer(32)


def val(buf):
    return int.from_bytes(buf.raw, "big")


FE_EDGES = [0, 1, 2, 7, P - 1, P - 2, N - 1, N, P, P + 1, ALL_ONES_LIMBS, 1 << 255, (1 << 255) - 1, P >> 1,
            0x3FFFFFF, 1 << 26, (1 << 234) - 1, 1 << 234, 2**256 - 2**32]


def test_field_ops_vs_integers(S):
    rng = random.Random(2)
    vals = FE_EDGES + [rng.randrange(2**256) for _ in range(40)]
    ops = [(0, lambda a, b: a * b % P), (1, lambda a, b: a * a % P), (2, lambda a, b: (a + b) % P),
           (3, lambda a, b: (a - b) % P), (4, lambda a, b: -a % P), (7, lambda a, b: a % P)]
    o = out32()
    for a in vals:
        for b in FE_EDGES[:12] + vals[-6:]:
            for op, f in ops:
                S.secpcheck_fe_op(op, b32(a), b32(b), o)
                assert val(o) == f(a, b), (op, hex(a), hex(b))
            assert S.secpcheck_fe_equal(b32(a), b32(b)) == (1 if (a - b) % P == 0 else 0)


def test_field_sqrt_inverse_and_bytes(S):
    rng = random.Random(3)
    o = out32()
    for a in FE_EDGES + [rng.randrange(P) for _ in range(20)]:
        S.secpcheck_fe_op(5, b32(a), b32(0), o)
        assert val(o) == pow(a % P, (P + 1) // 4, P)
        S.secpcheck_fe_op(6, b32(a), b32(0), o)
        assert val(o) == pow(a % P, P - 2, P)
        assert S.secpcheck_fe_from_be32(b32(a), o) == (1 if a < P else 0)
        assert val(o) == a % P


def test_field_dependent_chain(S):
    """1,000 dependent steps at the largest magnitudes the group formulas use,
    never normalised on the way: a wrong limb bound trips the assertions or
    the value."""
    rng = random.Random(4)
    o = out32()
    for a, t in [(P - 1, P - 1), (ALL_ONES_LIMBS, ALL_ONES_LIMBS), (rng.randrange(P), rng.randrange(P)), (0, 1)]:
        S.secpcheck_fe_chain(b32(a), b32(t), 1000, o)
        x, tt = a % P, t % P
        for _ in range(1000):
            tt = ((3 * tt - x) ** 2 * (tt + 5 * x) + x) % P
        assert val(o) == tt


def test_scalar_ops_vs_integers(S):
    rng = random.Random(5)
    edges = [0, 1, 2, N - 1, N - 2, N >> 1, (N >> 1) + 1, N, N + 1, 2**256 - 1, 2**256 - N, 1 << 128, (1 << 129) - 1]
    vals = edges + [rng.randrange(2**256) for _ in range(30)]
    o = out32()
    for a in vals:
        for b in vals:
            fl = S.secpcheck_sc_op(0, b32(a), b32(b), o)
            ar, br = (a - N if a >= N else a), (b - N if b >= N else b)  # one conditional subtraction, as the header
            if ar < N and br < N:
                assert val(o) == ar * br % N, (hex(a), hex(b))
            assert (fl & 1) == (1 if a < N else 0)
            assert ((fl >> 1) & 1) == (1 if ar == 0 else 0)
            assert ((fl >> 2) & 1) == (1 if ar > N >> 1 else 0)
    for a in edges + vals[-10:]:
        ar = a - N if a >= N else a
        if ar < N:
            S.secpcheck_sc_op(1, b32(a), b32(0), o)
            assert val(o) == pow(ar, N - 2, N)


def _group(S, op, a, la, b, lb):
    ox, oy = out32(), out32()
    ax, ay = (a if a is not R.INF else (0, 0))
    bx, by = (b if b is not R.INF else (0, 0))
    inf = S.secpcheck_group_op(op, b32(ax), b32(ay), b32(la), int(a is R.INF), b32(bx), b32(by), b32(lb),
                               int(b is R.INF), ox, oy)
    return R.INF if inf else (val(ox), val(oy))


def test_group_ops_vs_restatement(S):
    """Double, mixed and full addition on every kind of pair: generic, P = Q
    (in different Jacobian scalings), P = -Q, either operand infinity."""
    rng = random.Random(6)
    pts = [R.G, R.mul(2, R.G), R.mul(3, R.G), R.mul(N - 1, R.G), R.mul(N - 2, R.G)] + \
          [R.mul(rng.randrange(1, N), R.G) for _ in range(4)] + [R.INF]
    for a in pts:
        for b in pts:
            want = R.add_affine(a, b)
            la, lb = rng.randrange(1, P), rng.randrange(1, P)
            assert _group(S, 0, a, la, b, lb) == want
            assert _group(S, 0, a, 1, b, 1) == want
            assert _group(S, 1, a, la, b, 1) == want
        assert _group(S, 2, a, rng.randrange(1, P), R.INF, 1) == R.add_affine(a, a)
    for p in pts:
        assert R.on_curve(p)


def test_decompress_and_g_table(S):
    ox, oy = out32(), out32()
    for k in (1, 2, 3, 12345, N - 1):
        pt = R.mul(k, R.G)
        assert S.secpcheck_decompress(R.compress(pt), ox, oy) == 1 and (val(ox), val(oy)) == pt
        other = bytes([R.compress(pt)[0] ^ 1]) + R.compress(pt)[1:]
        assert S.secpcheck_decompress(other, ox, oy) == 1 and (val(ox), val(oy)) == (pt[0], P - pt[1])
    for bad in (b"\x04" + b32(R.GX), b"\x02" + b32(P), b"\x02" + b32(P + 1), b"\x03" + bytes(32)):
        assert S.secpcheck_decompress(bad, ox, oy) == 0
    tab = (ctypes.c_uint32 * 300)()
    S.secpcheck_g_table(tab)
    for j in range(1, 16):
        x = sum(tab[20 * (j - 1) + i] << (26 * i) for i in range(10))
        y = sum(tab[20 * (j - 1) + 10 + i] << (26 * i) for i in range(10))
        assert (x, y) == R.mul(j, R.G)


def test_golden_vectors(S, golden):
    vecs = golden("secp256k1_vectors.json")
    assert len(vecs) >= 400
    for v in vecs:
        pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        got = S.secpcheck_verify_msg(pk, len(pk), msg, len(msg), sig, len(sig))
        assert got == int(v["valid"]), v["name"]
        assert S.secpcheck_verify(pk, hashlib.sha256(msg).digest(), sig) == int(v["valid"]), v["name"]
    # other sizes verify false
    v = vecs[0]
    pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
    assert v["valid"] and S.secpcheck_verify_msg(pk, 33, msg, len(msg), sig[:63], 63) == 0
    assert S.secpcheck_verify_msg(pk[:32], 32, msg, len(msg), sig, 64) == 0
    assert S.secpcheck_verify_msg(pk + b"\0" * 32, 65, msg, len(msg), sig, 64) == 0


def test_golden_file_is_what_the_generator_writes():
    """The restatement agrees with every stored verdict (the generator also
    checks OpenSSL and the by-construction verdicts when it runs)."""
    import json
    with open(os.path.join(REPO, "tests", "golden", "secp256k1_vectors.json")) as f:
        vecs = json.load(f)
    for v in vecs[::7]:
        assert R.verify(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) == v["valid"]
