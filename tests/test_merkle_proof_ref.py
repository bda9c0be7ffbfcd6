"""The restatement of crypto/merkle/proof.go (tests/merkle_proof_ref.py), the
checker of the device proofs, pinned through the roots the reference holds
(tests/golden/merkle_vectors.json: crypto/merkle/tree_test.go:21-33 and
types/validator_set_test.go:51-53; the reference has no fixed proof vectors)
and checked against itself.  No GPU."""
import hashlib
import json
import os

import pytest

import merkle_ref as M
import merkle_proof_ref as P

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "merkle_vectors.json")))


def _golden_trees():
    for t in GOLD["tree"]:
        yield t["name"], [bytes.fromhex(x) for x in t["items"]], bytes.fromhex(t["hash"])
    sv = GOLD["simple_validator"]
    for s in GOLD["valsets"]:
        items = [M.simple_validator_bytes(bytes.fromhex(sv[i]["pk"]), sv[i]["kind"], sv[i]["power"])
                 for i in s["members"]]
        yield "valset %s" % s["members"], items, bytes.fromhex(s["hash"])


def test_proofs_compute_the_golden_roots():
    seen = 0
    for name, items, want in _golden_trees():
        root, proofs = P.proofs_from_byte_slices(items)
        assert root == want, name
        assert len(proofs) == len(items)
        for i, p in enumerate(proofs):
            assert (p.total, p.index) == (len(items), i)
            assert p.leaf_hash == M.leaf_hash(items[i])
            assert p.compute_root_hash() == want, (name, i)
            assert p.validate_basic() is None and p.verify(want, items[i]) is None
            assert len(p.aunts) == P.aunt_count(i, len(items))
            seen += 1
    assert seen > 20


def _items(n):
    return [hashlib.sha256(b"item %d of %d" % (i, n)).digest()[:1 + (i * 7 + n) % 5] for i in range(n)]


def test_every_proof_verifies_up_to_130_leaves():
    for n in range(1, 131):
        items = _items(n)
        root, proofs = P.proofs_from_byte_slices(items)
        assert root == M.hash_from_byte_slices(items)
        for i, p in enumerate(proofs):
            assert p.verify_status(root, items[i]) == (P.OK, p.leaf_hash, root), (n, i)


def _flips(b):
    for bit in range(8 * len(b)):
        m = bytearray(b)
        m[bit >> 3] ^= 1 << (bit & 7)
        yield bytes(m)


@pytest.mark.parametrize("lo", range(1, 131, 10))
def test_every_single_bit_flip_fails(lo):
    """Every bit of the leaf, the leaf hash, each aunt and the root, for every
    proof of every tree of 1..130 leaves (ten tree sizes per case)."""
    for n in range(lo, min(lo + 10, 131)):
        items = _items(n)
        root, proofs = P.proofs_from_byte_slices(items)
        root_flips = list(_flips(root))
        for p, leaf in zip(proofs, items):
            for m in _flips(leaf):
                assert p.verify_status(root, m)[0] == P.ERR_LEAF
            q = p.copy()
            for m in _flips(p.leaf_hash):
                q.leaf_hash = m
                assert q.verify_status(root, leaf)[0] == P.ERR_LEAF
            for m in root_flips:
                st, _, computed = p.verify_status(m, leaf)
                assert st == P.ERR_ROOT and computed == root
            for a in range(len(p.aunts)):
                q = p.copy()
                for m in _flips(p.aunts[a]):
                    q.aunts[a] = m
                    st, _, computed = q.verify_status(root, leaf)
                    assert st == P.ERR_ROOT and computed is not None and computed != root


def test_nil_roots_and_order_of_tests():
    items = _items(5)
    root, proofs = P.proofs_from_byte_slices(items)
    p = proofs[2]
    for total, index, aunts in [(5, 5, p.aunts), (0, 0, []), (0, 2, p.aunts), (5, 2, p.aunts[:-1]),
                                (5, 2, p.aunts + [root]), (1, 0, [root]), (2, 0, [])]:
        q = P.Proof(total, index, p.leaf_hash, aunts)
        assert q.compute_root_hash() is None
        assert q.verify_status(root, items[2])[0] == P.ERR_ROOT
        assert q.verify(root, items[2]) == "invalid root hash: wanted %s got " % root.hex().upper()
    assert P.Proof(-1, -1, p.leaf_hash, p.aunts).verify(root, items[2]) == "proof total must be positive"
    assert P.Proof(5, -1, p.leaf_hash, p.aunts).verify(root, b"x") == "proof index cannot be negative"
    assert P.Proof(5, 2, p.leaf_hash, p.aunts).verify(b"\0" * 32, b"x").startswith("invalid leaf hash: wanted ")
    assert P.Proof(-1, 0, b"", []).validate_basic() == "negative Total"
    assert P.Proof(1, -1, b"", []).validate_basic() == "negative Index"
    assert P.Proof(1, 0, b"abc", []).validate_basic() == "expected LeafHash size to be 32, got 3"
    assert P.Proof(1, 0, root, [root] * 101).validate_basic() == "expected no more than 100 aunts, got 101"
    assert P.Proof(1, 0, root, [root, b"ab"]).validate_basic() == "expected Aunts#1 size to be 32, got 2"


def test_txs_and_parts():
    txs = [b"tx %d" % i * (i + 1) for i in range(33)]
    root, proofs = P.txs_proofs(txs)
    assert root == P.txs_hash(txs)
    assert all(p.verify(root, hashlib.sha256(t).digest()) is None for p, t in zip(proofs, txs))
    assert P.txs_hash([]) == M.empty_hash()
    assert [len(x) for x in P.split_parts(b"a" * 10, 4)] == [4, 4, 2] and P.split_parts(b"", 4) == []
