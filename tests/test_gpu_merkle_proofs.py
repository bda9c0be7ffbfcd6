"""Merkle proofs on the device (tmv_merkle_proofs, tmv_merkle_verify_proofs;
merkle_proof_kernels.hip) against the recursive restatement of
crypto/merkle/proof.go (tests/merkle_proof_ref.py) and hashlib.  All
comparisons are exact bytes."""
import hashlib
import random

import numpy as np
import pytest

import merkle_ref as M
import merkle_proof_ref as P

from tendermint_amd import _native, chains

pytestmark = pytest.mark.gpu

SEG = 512  # kMerkleSegBytes: bytes of a leaf staged through LDS per round (csrc/merkle_proof.h)
PART = 65536
LPW = (8, 16, 32, 64)


def _bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


# ---- leaf hashing ----

@pytest.fixture(scope="module")
def leaf_items():
    """An odd-length leaf first (every later leaf starts unaligned), the block
    and padding edges, the staging-round and part-size edges, one leaf of
    200,001 bytes, shuffled, then three short leaves behind a long one."""
    rng = random.Random(5)
    lens = [0, 1, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128,
            SEG - 1, SEG, SEG + 1, PART - 1, PART, PART + 1, 200001]
    rng.shuffle(lens)
    lens = [3] + lens + [PART, 5, 0, 17]
    items = [_bytes(rng, n) for n in lens]
    want = np.frombuffer(b"".join(M.leaf_hash(x) for x in items), np.uint8).reshape(-1, 32)
    want_pre = np.frombuffer(b"".join(M.leaf_hash(hashlib.sha256(x).digest()) for x in items), np.uint8).reshape(-1, 32)
    data, off = chains.pack_items(items)
    assert any(int(o) % 16 for o in off[1:-1])
    return items, data, off, want, want_pre


def _leaf_hashes(ctx, data, off, flags):
    n = len(off) - 1
    _, leaves, _, _ = ctx.merkle_proofs(data, off, np.array([0, n], np.uint32), flags=flags, aunts=False)
    return leaves


@pytest.mark.parametrize("flags", [0, _native.TMV_MERKLE_LONG_LEAVES] + [_native.merkle_lpw(l) for l in LPW],
                         ids=["default", "long"] + ["lpw%d" % l for l in LPW])
def test_leaf_hashes(ctx, leaf_items, flags):
    _, data, off, want, _ = leaf_items
    got = _leaf_hashes(ctx, data, off, flags)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0].tolist()


@pytest.mark.parametrize("flags", [0] + [_native.merkle_lpw(l) for l in LPW], ids=["default"] + ["lpw%d" % l for l in LPW])
def test_leaf_hashes_prehashed(ctx, leaf_items, flags):
    _, data, off, _, want_pre = leaf_items
    got = _leaf_hashes(ctx, data, off, flags | _native.TMV_MERKLE_PREHASH)
    assert np.array_equal(got, want_pre), np.nonzero((got != want_pre).any(axis=1))[0].tolist()


def test_leaf_hashes_short_kernel_agrees(ctx, leaf_items):
    _, data, off, want, _ = leaf_items
    assert np.array_equal(_leaf_hashes(ctx, data, off, _native.TMV_MERKLE_SHORT_LEAVES), want)


# ---- proof generation ----

TREE_SIZES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1000]


@pytest.fixture(scope="module")
def forest():
    """Every tree size in one launch, with empty trees between non-empty ones;
    leaves of 0..100 bytes.  The restatement's roots and proofs, computed once."""
    rng = random.Random(6)
    sizes = []
    for k, n in enumerate(TREE_SIZES):
        sizes.append(n)
        if k % 3 == 1:
            sizes.extend([0] * (1 + k % 2))
    trees = [[_bytes(rng, rng.randrange(0, 101)) for _ in range(n)] for n in sizes]
    trees[sizes.index(2)][0] = b""  # an empty leaf inside a tree
    items = [x for t in trees for x in t]
    data, leaf_off = chains.pack_items(items)
    tree_off = np.zeros(len(sizes) + 1, np.uint32)
    tree_off[1:] = np.cumsum(sizes)
    ref = [P.proofs_from_byte_slices(t) for t in trees]
    return dict(sizes=sizes, trees=trees, items=items, data=data, leaf_off=leaf_off, tree_off=tree_off, ref=ref)


@pytest.mark.parametrize("flags", [0, _native.TMV_MERKLE_LONG_LEAVES], ids=["default", "long"])
def test_proofs_equal_the_restatement(ctx, forest, flags):
    f = forest
    roots, leaves, aoff, aunts = ctx.merkle_proofs(f["data"], f["leaf_off"], f["tree_off"], flags=flags)
    want_roots = b"".join(r for r, _ in f["ref"])
    assert roots.tobytes() == want_roots
    proofs = [p for _, ps in f["ref"] for p in ps]
    assert leaves.tobytes() == b"".join(p.leaf_hash for p in proofs)
    assert np.diff(aoff.astype(np.int64)).tolist() == [len(p.aunts) for p in proofs]
    assert aunts.tobytes() == b"".join(a for p in proofs for a in p.aunts)
    # the same roots from tmv_merkle_roots, and without the aunts
    assert ctx.merkle_roots(f["data"], f["leaf_off"], f["tree_off"]).tobytes() == want_roots
    r2, l2, a2, v2 = ctx.merkle_proofs(f["data"], f["leaf_off"], f["tree_off"], flags=flags, aunts=False)
    assert r2.tobytes() == want_roots and l2.tobytes() == leaves.tobytes() and a2 is None and v2 is None


# ---- proof verification ----

def _run_verify(ctx, cases, given=False, flags=0):
    """cases: [(Proof, root, leaf)] -> the engine's outputs and the restatement's."""
    n = len(cases)
    aoff = np.zeros(n + 1, np.uint32)
    aoff[1:] = np.cumsum([len(p.aunts) for p, _, _ in cases])
    aunts = np.frombuffer(b"".join(a for p, _, _ in cases for a in p.aunts), np.uint8)
    lh = np.frombuffer(b"".join(p.leaf_hash for p, _, _ in cases), np.uint8)
    rt = np.frombuffer(b"".join(r for _, r, _ in cases), np.uint8)
    data, loff = (None, None) if given else chains.pack_items([leaf for _, _, leaf in cases])
    ok, status, lcalc, rcalc, nil = ctx.merkle_verify_proofs([p.total for p, _, _ in cases],
                                                             [p.index for p, _, _ in cases], lh, aunts, aoff, rt,
                                                             data, loff, flags)
    want_st, want_l, want_r, want_nil = [], [], [], []
    for p, root, leaf in cases:
        st, leaf_h, computed = p.verify_status(root, leaf)
        if given:  # no leaf test: the reference's remaining tests in order
            leaf_h = p.leaf_hash
            st = (P.ERR_TOTAL if p.total < 0 else P.ERR_INDEX if p.index < 0
                  else P.OK if computed == root else P.ERR_ROOT)
        want_st.append(st)
        want_l.append(leaf_h)
        want_r.append(computed or b"\0" * 32)
        want_nil.append(1 if computed is None else 0)
    assert status.tolist() == want_st
    assert lcalc.tobytes() == b"".join(want_l)
    assert rcalc.tobytes() == b"".join(want_r)
    assert nil.tolist() == want_nil
    assert ok == all(s == 0 for s in want_st)
    return want_st


def _valid_cases(forest):
    return [(p, root, leaf) for (root, ps), t in zip(forest["ref"], forest["trees"]) for p, leaf in zip(ps, t)]


def test_valid_proofs_verify(ctx, forest):
    cases = _valid_cases(forest)
    assert set(_run_verify(ctx, cases)) == {0}
    assert set(_run_verify(ctx, cases, flags=_native.TMV_MERKLE_LONG_LEAVES)) == {0}
    assert set(_run_verify(ctx, cases, given=True)) == {0}


def _mutations(forest):
    rng = random.Random(7)
    out = []
    by_size = {len(t): (root, ps, t) for (root, ps), t in zip(forest["ref"], forest["trees"])}
    for n in (1, 2, 3, 5, 8, 9, 17, 129, 1000):
        root, ps, t = by_size[n]
        for i in sorted({0, n // 2, n - 1}):
            p, leaf = ps[i], t[i]

            def mut(**kw):
                q = p.copy()
                for k, v in kw.items():
                    setattr(q, k, v)
                return q
            out.append((p, root, leaf))                                       # good ones mixed in
            if p.aunts:
                a = rng.randrange(len(p.aunts))
                flipped = list(p.aunts)
                flipped[a] = bytes([flipped[a][0] ^ 0x10]) + flipped[a][1:]
                out.append((mut(aunts=flipped), root, leaf))                  # flipped aunt
                out.append((mut(aunts=p.aunts[:-1]), root, leaf))             # aunt dropped (top)
                out.append((mut(aunts=p.aunts[1:]), root, leaf))              # aunt dropped (leaf sibling)
            out.append((mut(aunts=p.aunts + [root]), root, leaf))             # aunt appended
            out.append((mut(index=i + 1), root, leaf))                        # index + 1 (index = total for the last)
            out.append((mut(index=i - 1), root, leaf))                        # index - 1 (-1 for the first)
            out.append((mut(index=n), root, leaf))                            # index = total
            out.append((mut(total=n + 1), root, leaf))
            out.append((mut(total=n - 1), root, leaf))                        # total = 0 for n = 1
            out.append((mut(total=0), root, leaf))
            out.append((mut(total=-1), root, leaf))
            out.append((mut(index=-1), root, leaf))
            out.append((mut(total=-1, index=-1), root, leaf))
            out.append((mut(total=1, index=0, aunts=[p.aunts[0] if p.aunts else root]), root, leaf))  # one aunt at total 1
            out.append((mut(total=1 << 62, index=i, aunts=[_bytes(rng, 32) for _ in range(62)]), root, leaf))
            out.append((mut(total=1 << 62, index=(1 << 62) - 1 - i, aunts=[_bytes(rng, 32) for _ in range(62)]),
                        root, leaf))
            out.append((mut(total=(1 << 63) - 1, index=(1 << 63) - 2, aunts=[_bytes(rng, 32) for _ in range(62)]),
                        root, leaf))
            out.append((mut(aunts=[_bytes(rng, 32) for _ in range(100)]), root, leaf))               # 100 aunts
            out.append((p, root, leaf + b"x"))                                # wrong leaf
            out.append((p, root, b""))
            out.append((p, root[:31] + bytes([root[31] ^ 1]), leaf))          # wrong root
            if n > 1:
                j = (i + 1) % n
                out.append((ps[j], root, leaf))                               # two leaves swapped
                out.append((p, root, t[j]))
    # a proof from another tree that still fits the path: accepted exactly when the restatement accepts
    root5, ps5, t5 = by_size[5]
    out.append((P.Proof(5, 1, ps5[0].leaf_hash, ps5[0].aunts), root5, t5[0]))
    out.append((P.Proof(8, 0, ps5[0].leaf_hash, ps5[0].aunts), root5, t5[0]))  # same depth, other total: still the root
    rng.shuffle(out)
    return out


def test_mutated_proofs(ctx, forest):
    cases = _mutations(forest)
    st = _run_verify(ctx, cases)
    assert {0, 1, 2, 3, 4} <= set(st)
    st_given = _run_verify(ctx, cases, given=True)
    assert {0, 1, 2, 4} <= set(st_given) and 3 not in st_given


# ---- part sets and transactions over the engine ----

@pytest.mark.parametrize("part_size", [PART, 4096])
def test_part_sets(ctx, part_size):
    """Blocks cut into parts as NewPartSetFromData does, one tree per block, straight through the engine
    (the host layer's calls are tests/test_gpu_part_sets.py)."""
    rng = random.Random(8)
    blocks = [_bytes(rng, n) for n in (0, 1, PART, PART + 1, 3 * PART + 17)]
    parts = [P.split_parts(b, part_size) for b in blocks]
    data, leaf_off = chains.pack_items([x for ps in parts for x in ps])
    tree_off = np.zeros(len(blocks) + 1, np.uint32)
    tree_off[1:] = np.cumsum([len(ps) for ps in parts])
    roots, leaves, aoff, aunts = ctx.merkle_proofs(data, leaf_off, tree_off)
    cases = []
    for t, ps in enumerate(parts):
        want_root, want = P.proofs_from_byte_slices(ps)
        assert bytes(roots[t]) == want_root
        got = chains.proofs_of_tree(len(ps), leaves, aoff, aunts, int(tree_off[t]))
        assert [(p.total, p.index, p.leaf_hash, p.aunts) for p in got] == \
               [(p.total, p.index, p.leaf_hash, p.aunts) for p in want]
        cases += [(p, want_root, part) for p, part in zip(want, ps)]
    assert bytes(roots[0]) == M.empty_hash()
    assert set(_run_verify(ctx, cases)) == {0}
    # a part with one flipped byte, a part carrying another part's proof
    p, root, part = cases[-2]
    bad = [(p, root, part[:100] + bytes([part[100] ^ 1]) + part[101:]), (cases[-1][0], root, part), cases[-2]]
    assert _run_verify(ctx, bad) == [P.ERR_LEAF, P.ERR_LEAF, P.OK]


@pytest.mark.parametrize("n", [0, 1, 2, 33])
def test_txs_hash_and_proofs(ctx, n):
    rng = random.Random(9 + n)
    txs = [_bytes(rng, rng.randrange(1, 700)) for _ in range(n)]
    want_root, want = P.txs_proofs(txs)
    assert chains.txs_hash(ctx, txs) == want_root == P.txs_hash(txs)
    root, proofs = chains.txs_proofs(ctx, txs)
    assert root == want_root and len(proofs) == n
    for p, w, tx in zip(proofs, want, txs):
        assert (p.total, p.index, p.leaf_hash, p.aunts) == (w.total, w.index, w.leaf_hash, w.aunts)
        assert w.leaf_hash == M.leaf_hash(hashlib.sha256(tx).digest())
    if n:
        cases = [(w, want_root, tx) for w, tx in zip(want, txs)]
        # the proof's leaf is SHA-256(tx): hashed on the device with the prehash flag
        n_ = len(cases)
        aoff = np.zeros(n_ + 1, np.uint32)
        aoff[1:] = np.cumsum([len(p.aunts) for p, _, _ in cases])
        data, loff = chains.pack_items(txs)
        ok, status, lcalc, rcalc, nil = ctx.merkle_verify_proofs(
            [p.total for p in want], [p.index for p in want],
            np.frombuffer(b"".join(p.leaf_hash for p in want), np.uint8),
            np.frombuffer(b"".join(a for p in want for a in p.aunts), np.uint8), aoff,
            np.frombuffer(want_root * n_, np.uint8), data, loff, _native.TMV_MERKLE_PREHASH)
        assert ok and not status.any() and not nil.any()
        assert rcalc.tobytes() == want_root * n_ and lcalc.tobytes() == b"".join(p.leaf_hash for p in want)


# ---- argument errors: TMV_ERR_ARG, nothing launched ----

def _arg_error(call):
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):
        call()


def test_argument_errors(ctx):
    data = np.arange(10, dtype=np.uint8)
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    for fn in (lambda lo, to, d=data: ctx.merkle_proofs(d, lo, to, aunts=False),
               lambda lo, to, d=data: ctx.merkle_roots(d, lo, to)):
        _arg_error(lambda: fn(u32(1, 5, 10), u32(0, 2)))            # non-zero first leaf offset
        _arg_error(lambda: fn(u32(0, 5, 10), u32(1, 2)))            # non-zero first tree offset
        _arg_error(lambda: fn(u32(0, 7, 5), u32(0, 2)))             # decreasing leaf offsets
        _arg_error(lambda: fn(u32(0, 3, 6, 10), u32(0, 2, 1, 3)))   # decreasing tree offsets
        _arg_error(lambda: fn(u32(0, 5, 10), u32(0, 1)))            # tree_off[n_trees] != n_leaves
        _arg_error(lambda: fn(u32(0, 5, 10), u32(0, 2), None))      # null data with bytes > 0
    # aunt offsets that are not the plan's
    lib, h = _native.lib(), ctx.handle
    lo, to = u32(0, 5, 10), u32(0, 2)
    roots, leaves, aunts = np.zeros(32, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    p = _native._p
    import ctypes
    c32 = ctypes.c_uint32
    assert lib.tmv_merkle_proofs(h, 0, p(data), p(lo, c32), 2, p(to, c32), 1, p(roots), p(leaves),
                                 p(u32(0, 1, 3), c32), p(aunts)) == _native.TMV_ERR_ARG
    assert lib.tmv_merkle_proofs(h, _native.TMV_MERKLE_LONG_LEAVES | _native.TMV_MERKLE_SHORT_LEAVES, p(data),
                                 p(lo, c32), 2, p(to, c32), 1, p(roots), p(leaves), None, None) == _native.TMV_ERR_ARG
    assert lib.tmv_merkle_proofs(h, _native.merkle_lpw(12), p(data), p(lo, c32), 2, p(to, c32), 1, p(roots),
                                 p(leaves), None, None) == _native.TMV_ERR_ARG
    # verification: the same checks on its offsets
    lh, rt = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    tot, idx = [2, 2], [0, 1]
    _arg_error(lambda: ctx.merkle_verify_proofs(tot, idx, lh, aunts, u32(1, 1, 2), rt, data, u32(0, 5, 10)))
    _arg_error(lambda: ctx.merkle_verify_proofs(tot, idx, lh, aunts, u32(0, 2, 1), rt, data, u32(0, 5, 10)))
    _arg_error(lambda: ctx.merkle_verify_proofs(tot, idx, lh, aunts, u32(0, 1, 2), rt, data, u32(1, 5, 10)))
    _arg_error(lambda: ctx.merkle_verify_proofs(tot, idx, lh, aunts, u32(0, 1, 2), rt, data, u32(0, 7, 5)))
    _arg_error(lambda: ctx.merkle_verify_proofs(tot, idx, lh, aunts, u32(0, 1, 2), rt, None, u32(0, 5, 10)))
    # and a well-formed call still runs afterwards
    assert ctx.merkle_roots(data, u32(0, 5, 10), u32(0, 2)).tobytes() == M.hash_from_byte_slices(
        [data[:5].tobytes(), data[5:].tobytes()])


def test_kernel_timing_names(ctx, forest):
    ctx.kernel_timing(True)
    try:
        f = forest
        ctx.merkle_proofs(f["data"], f["leaf_off"], f["tree_off"], flags=_native.TMV_MERKLE_LONG_LEAVES)
        for k in ("k_merkle_leaves_long", "k_merkle_tree_levels", "k_merkle_aunts"):
            ms, launches = ctx.kernel_timing_read(k)
            assert launches == 1 and ms > 0, k
    finally:
        ctx.kernel_timing(False)
