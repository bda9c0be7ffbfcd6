"""tests/golden/edge_forgeries.json on the CPU: inputs that are valid if and
only if one named rejection check is skipped (tests/golden/
make_edge_forgeries_golden.py builds them and proves that with a lax verifier
of its own), and the valid edges that must be accepted.  Every stored status
is the C oracle's and the Python restatement's, the device headers compiled
for the host give it too (the full equation and the half-size scalars), the
fixture holds every class it was built for, and the host layer's
BatchVerifier reports a key of every rejection class as the Add error it is.
No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ed25519_ref as E
import oracle_c as C
import sr25519_ref as S

import edge_forgeries_cases as F
from test_batch_verifier import cpu_backend  # noqa: F401  (fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "oracle", "_build", "libhostcheck.so")
P, L = E.P, E.L
ZERO32 = bytes(32)


@pytest.fixture(scope="module")
def H():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native")], check=True)
    return ctypes.CDLL(SO)


def p(a, t=ctypes.c_uint8):
    return a.ctypes.data_as(ctypes.POINTER(t))


def test_statuses_are_the_oracles(golden):
    """The C oracle on every record; the Python restatement on every seventh."""
    ed, sr = F.records(golden, "ed25519"), F.records(golden, "sr25519")
    assert len(ed) + len(sr) == len(F.records(golden)) and ed and sr
    _, vec = C.ed25519_verify_packed(*C.pack(F.entries(ed)))
    assert np.array_equal(vec.astype(np.int8), F.statuses(ed))
    st = C.sr25519_status_packed(*C.pack(F.entries(sr)))
    assert np.array_equal(st, F.statuses(sr))
    for v in ed[::7]:
        assert int(E.verify_zip215(*F.entry(v))) == v["status"], v["name"]
    for v in sr[::7]:
        pk, msg, sig = F.entry(v)
        try:
            S.batch_add_check(pk, sig)
            status = 1 if S.verify(pk, msg, sig) else 0
        except S.AddError as e:
            status = -1 if "public key" in str(e) else -2
        assert status == v["status"], v["name"]


def test_device_headers_on_the_host(H, golden):
    """The device's own decoding and equations, compiled for the host: the
    full verification and the half-size-scalar form of both schemes."""
    ed, sr = F.records(golden, "ed25519"), F.records(golden, "sr25519")
    pk, sig, msg, off = C.pack(F.entries(ed))
    out = np.zeros(len(ed), np.uint8)
    H.hostcheck_ed25519_verify_batch(p(pk), p(sig), p(msg), p(off, ctypes.c_uint32), len(ed), p(out))
    assert np.array_equal(out.astype(np.int8), F.statuses(ed))
    half = np.full(len(ed), -7, np.int8)
    slow = ctypes.c_int(0)
    H.hostcheck_verify_half(p(pk), p(sig), p(msg), p(off, ctypes.c_uint32), len(ed), 0, p(half, ctypes.c_int8),
                            ctypes.byref(slow))
    assert np.array_equal(half, F.statuses(ed))
    pk, sig, msg, off = C.pack(F.entries(sr))
    out = np.full(len(sr), -7, np.int8)
    H.hostcheck_sr25519_status_batch(p(pk), p(sig), p(msg), p(off, ctypes.c_uint32), len(sr), p(out, ctypes.c_int8))
    assert np.array_equal(out, F.statuses(sr))
    half = np.full(len(sr), -7, np.int8)
    H.hostcheck_verify_half(p(pk), p(sig), p(msg), p(off, ctypes.c_uint32), len(sr), 1, p(half, ctypes.c_int8),
                            ctypes.byref(slow))
    assert np.array_equal(half, F.statuses(sr))


def _by(vs, head):
    return [v for v in vs if F.name_parts(v)[0] == head]


def _scalar(v):
    return int.from_bytes(bytes.fromhex(v["sig"])[32:], "little")


def test_census_sr25519(golden):
    """Every class and tag the fixture was built for is there, in the numbers
    it was built with: a regenerated fixture cannot quietly lose one."""
    sr = F.records(golden, "sr25519")
    assert {v["skipped_check"] for v in sr} == {None, "key_ok", "key_sign", "key_neg_t", "key_bit255", "r_ok", "s_lt_l",
                                                "marker", "order_scalar_first", "order_r_first"}
    assert all((v["skipped_check"] is None) == (v["status"] == 1) for v in sr)
    marker = 1 << 255
    # rejected keys that act as the identity: every class, each key with s in {0, 1, random, l - 1}
    keys = {}
    for v in _by(sr, "key_identity"):
        assert v["skipped_check"] == "key_ok" and v["status"] == -1
        keys.setdefault((F.name_parts(v)[1], v["pk"]), set()).add(_scalar(v) - marker)
    per_class = {c: [k for (cc, k) in keys if cc == c] for c in F.SR_CLASSES}
    assert {c for c, _ in keys} == set(F.SR_CLASSES)
    for (c, k), scalars in keys.items():
        assert {0, 1, L - 1} < scalars and len(scalars) == 4, (c, k)
    assert len(per_class["nonsquare_flipped_i"]) >= 4 and len(per_class["nonsquare_none"]) >= 4
    as_int = lambda k: int.from_bytes(bytes.fromhex(k), "little")  # noqa: E731
    assert [as_int(k) for k in per_class["y_zero"]] == [P - 1]
    nc = {as_int(k) for k in per_class["noncanonical"]}
    assert {P, P + 18} <= nc and all(P <= x < 1 << 255 for x in nc)
    assert all(as_int(k) >> 255 == 1 and S.ristretto_decode((as_int(k) & (marker - 1)).to_bytes(32, "little"))
               for k in per_class["bit255"])
    assert all(as_int(k) & 1 for k in per_class["negative"])
    assert any(S.ristretto_decode((P - as_int(k)).to_bytes(32, "little")) for k in per_class["negative"])
    assert all(S.ristretto_decode(bytes.fromhex(k)) is None for _, k in keys)
    # rejected encodings of a signer's own point
    lax = _by(sr, "lax_key")
    for cls, tag, least in (("negative", "key_sign", 8), ("neg_t", "key_neg_t", 8), ("bit255", "key_bit255", 1)):
        got = [v for v in lax if F.name_parts(v)[1] == cls]
        assert len({v["pk"] for v in got}) >= least
        assert all(v["skipped_check"] == tag and v["status"] == -1 for v in got)
    # the valid keys decode through both of sqrt_ratio_i's accepting outcomes
    assert {F.name_parts(v)[3] for v in lax} == {"correct", "flipped"}
    # rejected R under the zero key with s = 0
    rs = _by(sr, "r_identity")
    assert {F.name_parts(v)[1] for v in rs} == set(F.SR_CLASSES)
    assert all(v["pk"] == ZERO32.hex() and _scalar(v) == marker and v["status"] == 0 and v["skipped_check"] == "r_ok"
               and S.ristretto_decode(bytes.fromhex(v["sig"])[:32]) is None for v in rs)
    # precedence and scalar edges
    got = {v["name"]: (v["skipped_check"], v["status"]) for v in _by(sr, "precedence") + _by(sr, "scalar")}
    assert got == {"precedence/bad_key_no_marker": ("order_scalar_first", -1),
                   "precedence/bad_key_s_eq_l": ("order_scalar_first", -1),
                   "precedence/s_eq_l_bad_r": ("order_r_first", -2),
                   "scalar/s_plus_l/0": ("s_lt_l", -2), "scalar/s_plus_l/1": ("s_lt_l", -2),
                   "scalar/no_marker/0": ("marker", -2), "scalar/no_marker/1": ("marker", -2)}
    # must accept
    zero = [v for v in _by(sr, "accept") if F.name_parts(v)[1] == "zero_key"]
    assert all(v["pk"] == ZERO32.hex() for v in zero) and {0, 1, L - 1} < {_scalar(v) - marker for v in zero}
    ident = [v for v in _by(sr, "accept") if F.name_parts(v)[1] == "r_identity"]
    assert len(ident) >= 2 and all(v["sig"][:64] == ZERO32.hex() and v["pk"] != ZERO32.hex() for v in ident)
    assert {F.name_parts(v)[3] for v in ident} == {"correct", "flipped"}


def test_census_ed25519(golden):
    ed = F.records(golden, "ed25519")
    assert {v["skipped_check"] for v in ed} == {None, "a_decode", "r_decode", "s_lt_l"}
    assert all((v["skipped_check"] is None) == (v["status"] == 1) for v in ed)
    keys = {}
    for v in _by(ed, "a_identity"):
        assert v["skipped_check"] == "a_decode" and v["status"] == 0
        keys.setdefault(v["pk"], set()).add(_scalar(v))
    assert len(keys) >= 8 and all(E.decode_point_zip215(bytes.fromhex(k)) is None for k in keys)
    assert all({0, 1, L - 1} < s and len(s) == 4 for s in keys.values())
    # among them: the sign bit set, and y >= p (reduced before the square root)
    assert any(int(k[62:], 16) & 0x80 for k in keys)
    assert any(int.from_bytes(bytes.fromhex(k), "little") & ((1 << 255) - 1) >= P for k in keys)
    per_a = {}
    for v in _by(ed, "r_identity"):
        assert v["skipped_check"] == "r_decode" and v["status"] == 0 and _scalar(v) == 0
        assert E.decode_point_zip215(bytes.fromhex(v["sig"])[:32]) is None
        per_a.setdefault(v["pk"], set()).add(v["sig"][:64])
    assert set(per_a) == {e.hex() for e in E.small_order_encodings()} and len(per_a) == 14
    assert all(len(r) >= 4 for r in per_a.values())
    sc = _by(ed, "scalar")
    assert {F.name_parts(v)[1] for v in sc} == {"s_plus_l", "s_plus_2l"}
    assert all(v["skipped_check"] == "s_lt_l" and v["status"] == 0 for v in sc)
    assert {_scalar(v) // L for v in sc} == {1, 2}
    # mixed order: [l] of the point is the torsion part (times l mod 8 = 5), of every order
    shapes = {}
    for v in _by(ed, "accept"):
        _, shape, t, signer = F.name_parts(v)
        shapes.setdefault(shape, set()).add((t, signer))
        pk, _, sig = F.entry(v)
        want = int(t.split("order")[1])
        for enc, mixed in ((sig[:32], shape != "mixed_a"), (pk, shape != "mixed_r")):
            T = E.pt_mul(L, E.decode_point_zip215(enc))
            order = next(o for o in (1, 2, 4, 8) if E.pt_is_identity(E.pt_mul(o, T)))
            assert order == (want if mixed else 1), v["name"]
    assert set(shapes) == {"mixed_r", "mixed_a", "mixed_both"}
    for got in shapes.values():
        assert len({t for t, _ in got}) == 8 and len(got) >= 16
        assert sorted(int(t.split("order")[1]) for t in {t for t, _ in got}) == [1, 2, 4, 4, 8, 8, 8, 8]


def test_fixture_is_no_larger_than_the_largest(golden):
    sizes = {f: os.path.getsize(os.path.join(REPO, "tests", "golden", f))
             for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.endswith(".json")}
    assert sizes["edge_forgeries.json"] <= max(v for f, v in sizes.items() if f != "edge_forgeries.json")


def test_generator_reproduces_the_fixture():
    """The committed fixture is what its generator writes, byte for byte, and
    the generator's own assertions hold: the restatement gives each stored
    status, and each record with a skipped check is accepted by the lax
    verifier that leaves only that check out."""
    import importlib.util
    path = os.path.join(REPO, "tests", "golden", "make_edge_forgeries_golden.py")
    spec = importlib.util.spec_from_file_location("make_edge_forgeries_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(REPO, "tests", "golden", "edge_forgeries.json")) as f:
        assert f.read() == gen.render()


def test_batch_verifier_rejected_keys_cpu(cpu_backend, golden):  # noqa: F811
    F.check_batch_verifier_rejected_keys(cpu_backend, golden)
