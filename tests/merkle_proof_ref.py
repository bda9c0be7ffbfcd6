"""CPU restatement of crypto/merkle/proof.go over hashlib (TEST INFRASTRUCTURE:
the checker for tmv_merkle_proofs / tmv_merkle_verify_proofs, never part of
the product path).

Follows the reference in its *recursive* form, so it shares no structure with
the iterative device code (level-by-level pairing, mask-and-fold):
  proof.go:33-48     ProofsFromByteSlices
  proof.go:52-68     Proof.Verify
  proof.go:98-117    Proof.ValidateBasic
  proof.go:151-181   computeHashFromAunts
  proof.go:197-215   ProofNode.FlattenAunts
  proof.go:219-239   trailsFromByteSlices
  types/tx.go:34-75  Txs.Hash / Txs.Proof (leaves are SHA-256(tx))
  types/part_set.go:172-200, 272-300  NewPartSetFromData, PartSet.AddPart
The reference holds no fixed proof vectors (proof_test.go and tree_test.go draw
random items), so proofs are pinned through the roots it does hold:
tests/test_merkle_proof_ref.py requires every restated proof of the trees in
tests/golden/merkle_vectors.json to compute the golden root.
"""
import functools
import hashlib
import sys

from merkle_ref import empty_hash, inner_hash, leaf_hash, split_point

sys.setrecursionlimit(10000)

MAX_AUNTS = 100  # proof.go:19
HASH_SIZE = 32

# Status of tmv_merkle_verify_proofs (include/tmverify.h)
OK, ERR_TOTAL, ERR_INDEX, ERR_LEAF, ERR_ROOT = 0, 1, 2, 3, 4
VERIFY_TEXT = {ERR_TOTAL: "proof total must be positive", ERR_INDEX: "proof index cannot be negative"}


_leaf_hash = functools.lru_cache(maxsize=1 << 12)(leaf_hash)


class ProofNode:
    def __init__(self, h):
        self.hash, self.parent, self.left, self.right = h, None, None, None

    def flatten_aunts(self):
        out, spn = [], self
        while spn is not None:
            if spn.left is not None:
                out.append(spn.left.hash)
            elif spn.right is not None:
                out.append(spn.right.hash)
            spn = spn.parent
        return out


def trails_from_byte_slices(items):
    n = len(items)
    if n == 0:
        return [], ProofNode(empty_hash())
    if n == 1:
        t = ProofNode(leaf_hash(items[0]))
        return [t], t
    k = split_point(n)
    lefts, left_root = trails_from_byte_slices(items[:k])
    rights, right_root = trails_from_byte_slices(items[k:])
    root = ProofNode(inner_hash(left_root.hash, right_root.hash))
    left_root.parent, left_root.right = root, right_root
    right_root.parent, right_root.left = root, left_root
    return lefts + rights, root


class Proof:
    def __init__(self, total, index, leaf_hash_, aunts):
        self.total, self.index, self.leaf_hash, self.aunts = total, index, leaf_hash_, list(aunts)

    def copy(self):
        return Proof(self.total, self.index, self.leaf_hash, self.aunts)

    def compute_root_hash(self):
        return compute_hash_from_aunts(self.index, self.total, self.leaf_hash, self.aunts)

    def verify_status(self, root, leaf, prehash=False):
        """(status, computed leaf hash, computed root or None) in Verify's order of tests."""
        lh = _leaf_hash(hashlib.sha256(leaf).digest() if prehash else leaf)
        computed = self.compute_root_hash()
        if self.total < 0:
            st = ERR_TOTAL
        elif self.index < 0:
            st = ERR_INDEX
        elif self.leaf_hash != lh:
            st = ERR_LEAF
        elif computed != root:  # a nil computed root equals no 32-byte root
            st = ERR_ROOT
        else:
            st = OK
        return st, lh, computed

    def verify(self, root, leaf):
        """Proof.Verify: None or the reference's error text."""
        st, lh, computed = self.verify_status(root, leaf)
        if st in VERIFY_TEXT:
            return VERIFY_TEXT[st]
        if st == ERR_LEAF:
            return "invalid leaf hash: wanted %s got %s" % (lh.hex().upper(), self.leaf_hash.hex().upper())
        if st == ERR_ROOT:
            return "invalid root hash: wanted %s got %s" % (root.hex().upper(), (computed or b"").hex().upper())
        return None

    def validate_basic(self):
        if self.total < 0:
            return "negative Total"
        if self.index < 0:
            return "negative Index"
        if len(self.leaf_hash) != HASH_SIZE:
            return "expected LeafHash size to be %d, got %d" % (HASH_SIZE, len(self.leaf_hash))
        if len(self.aunts) > MAX_AUNTS:
            return "expected no more than %d aunts, got %d" % (MAX_AUNTS, len(self.aunts))
        for i, a in enumerate(self.aunts):
            if len(a) != HASH_SIZE:
                return "expected Aunts#%d size to be %d, got %d" % (i, HASH_SIZE, len(a))
        return None


def proofs_from_byte_slices(items):
    trails, root = trails_from_byte_slices(items)
    return root.hash, [Proof(len(items), i, t.hash, t.flatten_aunts()) for i, t in enumerate(trails)]


def compute_hash_from_aunts(index, total, leaf_hash_, inner_hashes):
    return _hash_from_aunts(index, total, leaf_hash_, tuple(inner_hashes))


@functools.lru_cache(maxsize=1 << 14)
def _hash_from_aunts(index, total, leaf_hash_, inner_hashes):
    """computeHashFromAunts, recursive as the reference.  Memoised (a pure function of its arguments):
    proofs that differ in one aunt share the recursion below it, which the exhaustive bit-flip test needs."""
    if index >= total or index < 0 or total <= 0:
        return None
    if total == 1:
        return None if len(inner_hashes) != 0 else leaf_hash_
    if len(inner_hashes) == 0:
        return None
    num_left = split_point(total)
    if index < num_left:
        left = _hash_from_aunts(index, num_left, leaf_hash_, inner_hashes[:-1])
        return None if left is None else inner_hash(left, inner_hashes[-1])
    right = _hash_from_aunts(index - num_left, total - num_left, leaf_hash_, inner_hashes[:-1])
    return None if right is None else inner_hash(inner_hashes[-1], right)


def aunt_count(index, total):
    """Depth of leaf `index` in the split-point tree of `total` leaves, recursively."""
    if total <= 1:
        return 0
    k = split_point(total)
    return 1 + (aunt_count(index, k) if index < k else aunt_count(index - k, total - k))


def txs_hash(txs):
    from merkle_ref import hash_from_byte_slices
    return hash_from_byte_slices([hashlib.sha256(tx).digest() for tx in txs])


def txs_proofs(txs):
    return proofs_from_byte_slices([hashlib.sha256(tx).digest() for tx in txs])


def split_parts(data, part_size):
    """NewPartSetFromData's parts (types/part_set.go:172-186)."""
    total = (len(data) + part_size - 1) // part_size
    return [data[i * part_size:min(len(data), (i + 1) * part_size)] for i in range(total)]
