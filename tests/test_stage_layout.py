"""csrc/host/stage_layout.h (where the regions of a staged call sit, and the
offsets check of the synchronous entry points) through tests/native/stage,
against a restatement of its rules, and the same header under ASan + UBSan as
a stand-alone program.  No GPU; nothing sanitized is loaded into this
interpreter."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libstagecheck.so")
IN, PADDED, SCRATCH, OUT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    u8p, u32p, u64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
    L.sl_layout.restype = None
    L.sl_layout.argtypes = [u8p, u64p, u64p, ctypes.c_uint32, u64p, u64p]
    L.sl_check_offsets.argtypes = [u32p, ctypes.c_uint32, u32p]
    return L


def _layout(lib, regions):
    """regions: (kind, bytes[, spare]).  Returns the offsets and (in_bytes, out_at, out_bytes, dev_bytes, pad_at)."""
    kind = np.array([r[0] for r in regions], np.uint8)
    size = np.array([r[1] for r in regions], np.uint64)
    spare = np.array([r[2] if len(r) > 2 else 0 for r in regions], np.uint64)
    at, spans = np.zeros(len(regions), np.uint64), np.zeros(5, np.uint64)
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    lib.sl_layout(p(kind, ctypes.c_uint8), p(size, ctypes.c_uint64), p(spare, ctypes.c_uint64), len(regions),
                  p(at, ctypes.c_uint64), p(spans, ctypes.c_uint64))
    return [int(x) for x in at], tuple(int(x) for x in spans)


def _restated(regions):
    """The rules: every region from the next 16-byte boundary, in order; a padded one 16 bytes further."""
    a16 = lambda x: (x + 15) // 16 * 16
    cur, at, ends = 0, [], {IN: 0, SCRATCH: None, OUT: None}
    pad_at = 0
    for r in regions:
        kind, size, spare = r[0], r[1], (r[2] if len(r) > 2 else 0)
        if kind == PADDED:
            cur += 16
            pad_at = cur
        at.append(cur)
        cur += a16(size + spare)
        ends[IN if kind == PADDED else kind] = cur
    in_bytes = ends[IN]
    out_at = ends[SCRATCH] if ends[SCRATCH] is not None else in_bytes
    return at, (in_bytes, out_at, cur - out_at if ends[OUT] is not None else 0, cur, pad_at)


def _entry_point_shapes():
    """The region lists of the seven entry points, with counts that leave 8n, 4(n+1) and n off 16-byte boundaries."""
    for n, m, data in ((1, 1, 0), (5, 3, 5), (37, 9, 700), (1001, 37, 65537)):
        yield "valset", [(IN, 8 * n), (IN, 4 * (m + 1)), (IN, 32 * n), (IN, n), (SCRATCH, 32 * n), (SCRATCH, 32 * n),
                         (OUT, 32 * m)]
        yield "merkle roots", [(IN, 4 * (n + 1)), (IN, 4 * (m + 1)), (IN, data), (SCRATCH, 32 * n), (SCRATCH, 32 * n),
                               (OUT, 32 * m)]
        yield "commit", [(IN, 64 * n), (IN, 8 * n), (IN, 4 * n), (IN, 20 * n), (IN, 4 * (m + 1)), (IN, n), (IN, n),
                         (IN, n), (SCRATCH, 32 * n), (SCRATCH, 32 * n), (OUT, 32 * m)]
        for aunts in (0, 3 * n):
            yield "merkle proofs", [(IN, 4 * (n + 1)), (IN, 4 * (m + 1)), (IN, 4 * (n + 1) if aunts else 0),
                                    (PADDED, data), (SCRATCH, 32 * n), (SCRATCH, 32 * (n + 32 * m)), (OUT, 32 * m),
                                    (OUT, 32 * n), (OUT, 32 * aunts)]
            for given in (False, True):
                yield "merkle verify", [(IN, 8 * n), (IN, 8 * n), (IN, 32 * n), (IN, 32 * n), (IN, 32 * aunts),
                                        (IN, 4 * (n + 1)), (IN, 0 if given else 4 * (n + 1)),
                                        (PADDED, 0 if given else data), (SCRATCH, 0 if given else 32 * n),
                                        (OUT, 32 * n), (OUT, 32 * n), (OUT, n), (OUT, n)]
            yield "value ops", [(IN, 8 * n), (IN, 8 * n), (IN, 32 * n), (IN, 32 * m), (IN, 32 * aunts),
                                (IN, 4 * (n + 1)), (IN, 4 * (m + 1)), (IN, 4 * (n + 1)), (IN, 4 * (m + 1)),
                                (IN, 33 * n), (PADDED, data), (OUT, 32 * n), (OUT, 32 * n), (OUT, 32 * m), (OUT, n),
                                (OUT, n), (OUT, m), (OUT, 4 * m)]
        for cache, miss in ((False, 0), (True, 0), (True, m)):
            yield "secp256k1", [(IN, 0 if cache else 48 * n), (IN, 64 * n), (IN, 4 * (n + 1)), (IN, data),
                                (IN, 4 * n if cache else 0), (IN, 48 * miss), (IN, 4 * miss), (OUT, n), (OUT, 4 * miss)]


def test_entry_point_layouts_equal_the_restatement(lib):
    for name, regions in _entry_point_shapes():
        at, spans = _layout(lib, regions)
        assert (at, spans) == _restated(regions), name
        in_bytes, out_at, out_bytes, dev_bytes, pad_at = spans
        assert in_bytes <= out_at and out_at + out_bytes == dev_bytes, name
        ends = [a + r[1] for a, r in zip(at, regions)]
        assert all(a % 16 == 0 for a in at) and all(e <= a for e, a in zip(ends, at[1:])), name
        for a, r in zip(at, regions):
            if r[0] == PADDED:
                assert pad_at == a and a - 16 >= max([e for e, b in zip(ends, at) if b < a], default=0), name
                assert a + r[1] <= in_bytes, name


def test_spare_bytes_stay_inside_the_region(lib):
    at, spans = _layout(lib, [(IN, 13, 3), (IN, 13, 4), (IN, 1)])
    assert at == [0, 16, 48] and spans[0] == 64


def test_check_offsets(lib):
    def run(off, n):
        a = np.array(off, np.uint32)
        span = ctypes.c_uint32(77)
        rc = lib.sl_check_offsets(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, ctypes.byref(span))
        return rc, span.value
    assert run([0, 3, 3, 10, 12], 4) == (0, 7)
    assert run([0], 0) == (0, 0)
    assert run([5], 0) == (1, 77)
    assert run([1, 2, 3], 2) == (1, 77)
    assert run([0, 5, 4, 9], 3) == (2, 77)
    assert run([2, 1], 1) == (1, 77)
    assert run([0, 2 ** 32 - 1], 1) == (0, 2 ** 32 - 1)
    rng = np.random.default_rng(5)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 1000, 4097))])
    assert run(off, 4097) == (0, int(np.diff(off).max()))
    off[2000] -= 1 + int(off[2000] - off[1999])
    assert run(off, 4097) == (2, 77)


def test_layout_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "stage"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "stage_san")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1:] == ["0 wrong"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
