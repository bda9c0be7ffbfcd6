"""Cases of the host layer's part-set and proof entry points (include/tmhost.h:
tmv_part_set_headers, tmv_part_set_proofs, tmv_parts_verify,
tmv_proofs_verify), shared by the CPU test of the host fallback
(tests/test_merkle_host.py, the layer built without the engine) and the GPU
test of the device path (tests/test_gpu_part_sets.py).  Expected results come
from the restatement of the reference (tests/merkle_proof_ref.py)."""
import random

import merkle_ref as M
import merkle_proof_ref as P

from tendermint_amd import host as H

PART = 65536
BLOCK_SIZES = (0, 1, PART, PART + 1, 2 * PART + 1, 3 * PART + 17)  # 2 PART + 1: its last part has one aunt


def _bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


_BLOCKS = None


def blocks():
    global _BLOCKS
    if _BLOCKS is None:
        rng = random.Random(8)
        _BLOCKS = [_bytes(rng, n) for n in BLOCK_SIZES]
    return _BLOCKS


def _h(p):
    return H.Proof(p.total, p.index, p.leaf_hash, list(p.aunts))


def add_part(part, total, hash_):
    """PartSet.AddPart's checks (types/part_set.go:272-300), restated."""
    if part.index >= total:
        return H.PART_ERR_UNEXPECTED_INDEX, "error part set unexpected index"
    pr = part.proof
    if P.Proof(pr.total, pr.index, pr.leaf_hash, pr.aunts).verify(hash_, part.bytes) is not None:
        return H.PART_ERR_INVALID_PROOF, "error part set invalid proof"
    return H.PART_OK, None


def check_part_sets(ctx, lib, part_size):
    bl = blocks()
    heads = H.part_set_headers(ctx, bl, part_size, lib=lib)
    got = H.part_set_proofs(ctx, bl, part_size, lib=lib)
    offered = []
    sets = []
    for b, head, (total, root, proofs) in zip(bl, heads, got):
        parts = P.split_parts(b, part_size)
        want_root, want = P.proofs_from_byte_slices(parts)
        assert head == (len(parts), want_root) == (total, root)
        assert [(p.total, p.index, p.leaf_hash, p.aunts) for p in proofs] == \
               [(p.total, p.index, p.leaf_hash, p.aunts) for p in want]
        sets.append((parts, want_root, want))
        offered += [(H.Part(i, x, _h(p)), len(parts), want_root) for i, (x, p) in enumerate(zip(parts, want))]
    assert heads[0] == (0, M.empty_hash())
    n_good = len(offered)
    parts, root, proofs = sets[-1]
    total = len(parts)
    x = parts[1]
    offered += [
        (H.Part(1, x[:9] + bytes([x[9] ^ 0x40]) + x[10:], _h(proofs[1])), total, root),   # one flipped byte
        (H.Part(1, x, _h(proofs[2])), total, root),                                       # another part's proof
        (H.Part(total, x, _h(proofs[1])), total, root),                                   # index = total
        (H.Part(total + 7, x, _h(proofs[1])), total, root),
        (H.Part(0, x, _h(proofs[1])), total, root),               # part.Index is not compared with proof.Index
        (H.Part(1, x, H.Proof(total + 1, 1, proofs[1].leaf_hash, proofs[1].aunts)), total, root),
        (H.Part(1, x, H.Proof(total, 1, proofs[1].leaf_hash[:31], proofs[1].aunts)), total, root),
        (H.Part(1, x, H.Proof(total, 1, proofs[1].leaf_hash, [a[:31] for a in proofs[1].aunts])), total, root),
        (H.Part(1, x, H.Proof(-1, 1, proofs[1].leaf_hash, proofs[1].aunts)), total, root),
        (H.Part(1, x, H.Proof(total, -1, proofs[1].leaf_hash, proofs[1].aunts)), total, root),
        (H.Part(1, x, _h(proofs[1])), total, root[:31] + bytes([root[31] ^ 1])),
        (H.Part(1, x, _h(proofs[1])), total, root[:20]),
    ]
    # a wrong proof.Index / proof.Total whose aunts still verify: the last part of the 2 PART + 1 block hangs
    # directly under the root (3 or 33 parts: 2^k + 1), as index 1 of a tree of 2 does
    parts1, root1, proofs1 = sets[-2]
    last = proofs1[-1]
    assert len(last.aunts) == 1 and len(parts1) > 2
    offered.append((H.Part(len(parts1) - 1, parts1[-1], H.Proof(2, 1, last.leaf_hash, last.aunts)), len(parts1), root1))
    # and the first part of the last block under a total of 2^depth that is not its set's
    depth = len(proofs[0].aunts)
    assert (1 << depth) != total or part_size == PART
    offered.append((H.Part(0, parts[0], H.Proof(1 << depth, 0, proofs[0].leaf_hash, proofs[0].aunts)), total, root))
    res = H.parts_verify(ctx, offered, lib=lib)
    want = [add_part(*o) for o in offered]
    assert res == want
    assert all(r == (H.PART_OK, None) for r in res[:n_good])
    kinds = {r[0] for r in res[n_good:]}
    assert kinds == {H.PART_OK, H.PART_ERR_UNEXPECTED_INDEX, H.PART_ERR_INVALID_PROOF}
    assert res[-1] == (H.PART_OK, None) and res[-2] == (H.PART_OK, None)


def check_proofs_verify(ctx, lib, big=False):
    """Every text of Proof.ValidateBasic and Proof.Verify; big: leaves of 64 KiB
    parts (the device path's size), else short ones."""
    rng = random.Random(10)
    items = [_bytes(rng, (PART if big else 40) + i) for i in range(11)]
    root, proofs = P.proofs_from_byte_slices(items)
    h32 = _bytes(rng, 32)
    p = proofs[6]
    table = [(pr, items[i], root) for i, pr in enumerate(proofs)]
    table += [
        (P.Proof(-1, 6, p.leaf_hash, p.aunts), items[6], root),           # negative Total
        (P.Proof(11, -1, p.leaf_hash, p.aunts), items[6], root),          # negative Index
        (P.Proof(11, 6, p.leaf_hash[:31], p.aunts), items[6], root),      # LeafHash size
        (P.Proof(11, 6, b"", p.aunts), items[6], root),
        (P.Proof(11, 6, p.leaf_hash, [h32] * 101), items[6], root),       # more than 100 aunts
        (P.Proof(11, 6, p.leaf_hash, p.aunts[:2] + [h32[:7]] + p.aunts[3:]), items[6], root),  # Aunts#2 size
        (P.Proof(11, 6, p.leaf_hash, p.aunts), items[5], root),           # invalid leaf hash
        (P.Proof(11, 6, h32, p.aunts), items[6], root),
        (P.Proof(11, 6, p.leaf_hash, p.aunts), items[6], h32),            # invalid root hash
        (P.Proof(11, 6, p.leaf_hash, p.aunts), items[6], root[:5]),
        (P.Proof(11, 6, p.leaf_hash, p.aunts), items[6], b""),
        (P.Proof(11, 6, p.leaf_hash, [h32] + p.aunts[1:]), items[6], root),
        (P.Proof(11, 6, p.leaf_hash, p.aunts[:-1]), items[6], root),      # nil computed root: "got " and nothing
        (P.Proof(11, 6, p.leaf_hash, p.aunts + [h32]), items[6], root),
        (P.Proof(11, 11, p.leaf_hash, p.aunts), items[6], root),
        (P.Proof(0, 0, p.leaf_hash, []), items[6], root),
        (P.Proof(1, 0, p.leaf_hash, [h32]), items[6], root),
        (P.Proof(11, 6, p.leaf_hash, [h32] * 100), items[6], root),       # 100 aunts pass ValidateBasic
        (P.Proof(1 << 62, 5, p.leaf_hash, [h32] * 62), items[6], root),
        (P.Proof(1, 0, p.leaf_hash, []), items[6], p.leaf_hash),          # a tree of one leaf
    ]
    want = [pr.validate_basic() or pr.verify(rt, leaf) for pr, leaf, rt in table]
    got = H.proofs_verify(ctx, [(_h(pr), leaf, rt) for pr, leaf, rt in table], lib=lib)
    assert got == want
    assert all(w is None for w in want[:11]) and want[-1] is None
    for text in ("negative Total", "negative Index", "expected LeafHash size to be 32, got 31",
                 "expected LeafHash size to be 32, got 0", "expected no more than 100 aunts, got 101",
                 "expected Aunts#2 size to be 32, got 7"):
        assert text in want
    assert sum(1 for w in want if w and w.startswith("invalid leaf hash: wanted ")) == 2
    assert sum(1 for w in want if w and w.startswith("invalid root hash: wanted ")) >= 9
    assert any(w and w.endswith(" got ") for w in want)
    # Verify's own first two texts ("proof total must be positive", "proof index cannot be negative")
    # cannot appear here, as in the reference: ValidateBasic rejects those proofs first.
