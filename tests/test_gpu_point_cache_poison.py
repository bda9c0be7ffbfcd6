"""Poisoned point cache (point_cache.h: a hit is checked, never trusted).  The
-DTMV_CHECKS test build (tendermint_amd/_build_checks/libtmgpu.so) alone has
the hooks that read and overwrite the device table; after a warm call the
table is filled in turn with random bytes, the right keys with x negated,
the right keys with another key's x, and x = 0 throughout.  The next call's
vector must equal the oracle's every time, and every poisoned entry must be
counted as a miss.  Runs in a subprocess (the library path is read at
import)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS_SO = os.path.join(ROOT, "tendermint_amd", "_build_checks", "libtmgpu.so")

CODE = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, '.'); sys.path.insert(0, 'oracle'); sys.path.insert(0, 'tests')
os.environ["TMV_POINT_CACHE_SLOTS"] = "16384"
from tendermint_amd import _native as N
import point_cache_cases as K
L = N.lib()
u8p = ctypes.POINTER(ctypes.c_uint8)
L.tmv_internal_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
L.tmv_internal_point_cache_read.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64]
L.tmv_internal_point_cache_write.argtypes = [ctypes.c_void_p, u8p, ctypes.c_uint64]
assert L.tmv_internal_option(b"point_cache_min", 512) == 0
P = 2**255 - 19
SLOTS = 16384
ctx = N.Context(1)
case = K.plain_case()

def verify():
    s0 = ctx.point_cache_stats()
    ok, st = ctx.verify_batch_ex(N.TMV_KIND_ED25519, N.TMV_FLAG_BATCH_EQUATION, case.pk, case.sig, case.msg, case.off)
    s1 = ctx.point_cache_stats()
    assert np.array_equal(np.asarray(st).astype(np.uint8), case.ref)
    return s1["hits"] - s0["hits"], s1["misses"] - s0["misses"]

def read():
    t = np.zeros(SLOTS * 64, np.uint8)
    assert L.tmv_internal_point_cache_read(ctx._h, t.ctypes.data_as(u8p), t.nbytes) == 0
    return t.reshape(SLOTS, 64)

def write(t):
    t = np.ascontiguousarray(t.reshape(-1))
    assert L.tmv_internal_point_cache_write(ctx._h, t.ctypes.data_as(u8p), t.nbytes) == 0

assert verify() == (0, case.n)                       # cold
hits, misses = verify()                              # warm: the table is used
assert hits > case.n // 2 and hits + misses == case.n and misses >= int((~case.decodable).sum())
good = read()
used = np.flatnonzero(good.any(axis=1))
assert len(used) > 500
# every entry the table holds is a decoded key with its x (x != 0 for these keys)
keys = set(case.keys)
for s in used[:50]:
    assert bytes(good[s, :32]) in keys and int.from_bytes(bytes(good[s, 32:]), "little") not in (0,)

rng = np.random.default_rng(3)
def neg_x(t):
    for s in used:
        x = int.from_bytes(bytes(t[s, 32:]), "little")
        t[s, 32:] = np.frombuffer(((P - x) % P).to_bytes(32, "little"), np.uint8)
def other_x(t):
    t[used, 32:] = good[np.roll(used, 1), 32:]
def zero_x(t):
    t[:, 32:] = 0
def rand(t):
    t[:] = rng.integers(0, 256, t.shape, dtype=np.uint8)
for name, poison in (("random", rand), ("negated x", neg_x), ("another key's x", other_x), ("x = 0", zero_x)):
    t = good.copy()
    poison(t)
    write(t)
    assert verify() == (0, case.n), name               # exact vector (in verify), every entry a miss
    assert verify()[0] > case.n // 2, name             # the miss pass put the right entries back
print("ok", hits, misses, len(used))
"""


def test_poisoned_table_is_never_trusted():
    assert os.path.exists(CHECKS_SO), f"{CHECKS_SO} missing: run tools/build_checks.sh (__graft_entry__.build() does)"
    env = dict(os.environ, TMV_LIB_PATH=CHECKS_SO)
    out = subprocess.run([sys.executable, "-c", CODE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "ok" in out.stdout


def test_product_build_has_no_table_hooks():
    import ctypes
    from tendermint_amd import _native as N
    L = N.lib()
    assert not hasattr(L, "tmv_internal_point_cache_write") and not hasattr(L, "tmv_internal_point_cache_read")
