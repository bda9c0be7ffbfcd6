"""CPU restatement of the reference's value proof operators and tx proofs over
hashlib (TEST INFRASTRUCTURE: the checker for tmv_merkle_value_ops,
tmv_proof_ops_verify and tmv_tx_proofs_validate, never part of the product
path), on top of tests/merkle_proof_ref.py:
  crypto/merkle/proof_value.go:77-98    ValueOp.Run
  crypto/merkle/proof_op.go:39-69       ProofOperators.Verify
  crypto/merkle/proof_op.go:102-130     ProofRuntime.DecodeProof / Verify (the error wrapping)
  crypto/merkle/proof.go:133-146        ProofFromProto (ValidateBasic on decoding)
  crypto/merkle/types.go                encodeByteSlice
  types/tx.go:286-301                   TxProof.Validate
The reference holds no "simple:v" vector (TestProofOperators uses a test-only
op), so parity with it rests on this restatement: unpinned by reference-held
vectors.  Go's nil and empty slices are both b"" here except where the
difference shows: args is None for VerifyAbsence, and a nil computed root is
None until it is passed on or compared (bytes.Equal(nil, []byte{}) is true;
%X prints nothing for either).
"""
import hashlib

import merkle_proof_ref as P
from merkle_ref import leaf_hash

DECODE_PREFIX = "decoding proof: decoding a proof operator: "


def uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def encode_byte_slice(b):
    return uvarint(len(b)) + b


def kv_bytes(key, value):
    return encode_byte_slice(key) + encode_byte_slice(hashlib.sha256(value).digest())


class ValueOp:
    def __init__(self, key, proof):
        self.key, self.proof = key, proof

    def kv_hash(self, value):
        return leaf_hash(kv_bytes(self.key, value))

    def run(self, args):
        """ValueOp.Run: (args, None) or (None, error text)."""
        if args is None or len(args) != 1:
            return None, "expected 1 arg, got %d" % (0 if args is None else len(args))
        kvhash = self.kv_hash(args[0])
        if kvhash != self.proof.leaf_hash:
            return None, "leaf hash mismatch: want %s got %s" % (self.proof.leaf_hash.hex().upper(), kvhash.hex().upper())
        return [self.proof.compute_root_hash() or b""], None  # a nil root is hashed as the empty string by the next op


def _s(b):
    """Go's string(b) printed with %+v: the raw bytes."""
    return b.decode("latin-1")


def operators_verify(ops, root, keys, args):
    """ProofOperators.Verify with keys = KeyPathToKeys(keypath): None or the error text."""
    keys = list(keys)
    for i, op in enumerate(ops):
        if len(op.key) != 0:
            if len(keys) == 0:
                return "key path has insufficient # of parts: expected no more keys but got %s" % _s(op.key)
            last = keys[-1]
            if last != op.key:
                return "key mismatch on operation #%d: expected %s but got %s" % (i, _s(last), _s(op.key))
            keys.pop()
        args, err = op.run(args)
        if err is not None:
            return err
    if args is None:
        raise IndexError("args[0] of nil: the reference panics")
    if root != args[0]:
        return "calculated root hash is invalid: expected %s but got %s" % (root.hex().upper(), args[0].hex().upper())
    if len(keys) != 0:
        return "keypath not consumed all"
    return None


def runtime_verify(ops, root, keys, value):
    """ProofRuntime.Verify under DefaultProofRuntime for decoded "simple:v" ops; value None = VerifyAbsence."""
    for op in ops:  # DecodeProof: every op's ProofFromProto before anything runs
        err = op.proof.validate_basic()
        if err is not None:
            return DECODE_PREFIX + err
    return operators_verify(ops, root, keys, None if value is None else [value])


def tx_proof_validate(root_hash, data, proof, data_hash):
    """TxProof.Validate(dataHash): None or the error text."""
    if data_hash != root_hash:
        return "proof matches different data hash"
    if proof.index < 0:
        return "proof index cannot be negative"
    if proof.total <= 0:
        return "proof total must be positive"
    leaf = hashlib.sha256(data).digest()  # Tx.Hash
    # Proof.Verify (proof.go:52-68); a nil computed root equals an empty RootHash (bytes.Equal)
    if proof.leaf_hash != leaf_hash(leaf) or (proof.compute_root_hash() or b"") != root_hash:
        return "proof is not internally consistent"
    return None


def engine_expect(value, ops, root):
    """What tmv_merkle_value_ops computes for one item: per op (kv hash, leaf_ok, root or None), then
    (status, fail_op)."""
    per_op, v, first_bad = [], value, None
    for j, op in enumerate(ops):
        kv = op.kv_hash(v)
        r = op.proof.compute_root_hash()
        per_op.append((kv, kv == op.proof.leaf_hash, r))
        if kv != op.proof.leaf_hash and first_bad is None:
            first_bad = j
        v = r or b""
    last = per_op[-1][2]
    if first_bad is not None:
        return per_op, (P.ERR_LEAF, first_bad)
    if last is None or last != root:
        return per_op, (P.ERR_ROOT, len(ops) - 1)
    return per_op, (P.OK, 0)
