"""Cases of tmv_proof_ops_verify and tmv_tx_proofs_validate (include/tmhost.h),
shared by the CPU test of the host path (tests/test_proof_ops_host.py, the
layer built without the engine), the GPU test of the device path
(tests/test_gpu_proof_ops.py) and the golden file's generator
(tests/golden/make_proof_ops_golden.py).  Expected texts come from the
restatement of the reference (tests/proof_ops_ref.py); every named case also
states the text it must end in, so the sequencing is pinned twice."""
import json
import random

import merkle_proof_ref as P
import proof_ops_ref as R

from tendermint_amd import host as H
from tendermint_amd.testing import simple_map as SM

ERR_CUT = H.ERR_STRIDE - 1  # texts are cut to the stride


def _bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def _pairs(rng, n, tag):
    return {b"%s/key-%03d" % (tag, i): _bytes(rng, 8 + i % 5) for i in range(n)}


def _ref_ops(item):
    return [R.ValueOp(op.key, P.Proof(op.proof.total, op.proof.index, op.proof.leaf_hash, op.proof.aunts))
            for op in item.ops]


def expected(item):
    text = R.runtime_verify(_ref_ops(item), item.root, item.keys, item.value)
    return None if text is None else text[:ERR_CUT]


def _with(item, **kw):
    d = dict(ops=list(item.ops), root=item.root, keys=list(item.keys), value=item.value)
    d.update(kw)
    return H.ProofOpsItem(**d)


def _op(op, **kw):
    d = dict(total=op.proof.total, index=op.proof.index, leaf_hash=op.proof.leaf_hash, aunts=list(op.proof.aunts))
    key = kw.pop("key", op.key)
    d.update(kw)
    return H.ValueOp(key, H.Proof(**d))


_CASES = None


def proof_ops_cases():
    """[(name, item, what the text must start with or None for ok)]."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = random.Random(19)
    gen = P.proofs_from_byte_slices
    store = _pairs(rng, 11, b"bank")
    multi = _pairs(rng, 5, b"store")
    top = _pairs(rng, 3, b"app")
    one = SM.nested([(store, b"bank/key-004")], gen)
    two = SM.nested([(store, b"bank/key-004"), (multi, b"bank")], gen)
    three = SM.nested([(store, b"bank/key-010"), (multi, b"bank"), (top, b"root")], gen)
    single = SM.nested([({b"only": b""}, b"only")], gen)  # a tree of one leaf, an empty value
    h32 = _bytes(rng, 32)
    o0, o1 = two.ops
    cases = [
        ("ok 1 op", one, None),
        ("ok 2 ops", two, None),
        ("ok 3 ops", three, None),
        ("ok one-leaf tree, empty value", single, None),
        # TestProofOperators' sequencing (crypto/merkle/proof_test.go:67-138) with value ops
        ("too few keys", _with(two, keys=two.keys[1:]), "key path has insufficient # of parts: expected no more keys but got bank"),
        ("no keys", _with(two, keys=[]), "key path has insufficient # of parts: expected no more keys but got bank/key-004"),
        ("too many keys", _with(two, keys=[b"extra"] + two.keys), "keypath not consumed all"),
        ("wrong key at op 0", _with(two, keys=[two.keys[0], b"bank/key-005"]),
         "key mismatch on operation #0: expected bank/key-005 but got bank/key-004"),
        ("wrong key at op 1", _with(two, keys=[b"bonk", two.keys[1]]),
         "key mismatch on operation #1: expected bonk but got bank"),
        ("keys in the wrong order", _with(two, keys=two.keys[::-1]), "key mismatch on operation #0: expected bank but got"),
        ("wrong value", _with(two, value=b"another"), "leaf hash mismatch: want " + o0.proof.leaf_hash.hex().upper() + " got "),
        ("wrong root", _with(two, root=h32), "calculated root hash is invalid: expected " + h32.hex().upper() + " but got "
         + two.root.hex().upper()),
        # ValidateBasic of every op runs before anything else
        ("ValidateBasic at op 1 wins over a key mismatch at op 0",
         _with(two, ops=[o0, _op(o1, leaf_hash=o1.proof.leaf_hash[:31])], keys=[b"bank", b"nope"]),
         R.DECODE_PREFIX + "expected LeafHash size to be 32, got 31"),
        ("ValidateBasic: negative Total", _with(one, ops=[_op(one.ops[0], total=-1)]), R.DECODE_PREFIX + "negative Total"),
        ("ValidateBasic: negative Index", _with(one, ops=[_op(one.ops[0], index=-1)]), R.DECODE_PREFIX + "negative Index"),
        ("ValidateBasic: 101 aunts", _with(one, ops=[_op(one.ops[0], aunts=[h32] * 101)]),
         R.DECODE_PREFIX + "expected no more than 100 aunts, got 101"),
        ("ValidateBasic: aunt size", _with(one, ops=[_op(one.ops[0], aunts=[h32, h32[:5]])]),
         R.DECODE_PREFIX + "expected Aunts#1 size to be 32, got 5"),
        ("ValidateBasic wins over absence", _with(one, ops=[_op(one.ops[0], leaf_hash=b"")], value=None),
         R.DECODE_PREFIX + "expected LeafHash size to be 32, got 0"),
        ("a leaf mismatch at op 0 hides a key mismatch at op 1", _with(two, value=b"x", keys=[b"nope", two.keys[1]]),
         "leaf hash mismatch: want "),
        ("a key mismatch at op 0 hides a leaf mismatch at op 0", _with(two, value=b"x", keys=[two.keys[0], b"nope"]),
         "key mismatch on operation #0"),
        ("leaf mismatch at op 1 (a flipped aunt of op 0)",
         _with(two, ops=[_op(o0, aunts=[h32] + o0.proof.aunts[1:]), o1]), "leaf hash mismatch: want " + o1.proof.leaf_hash.hex().upper()),
        ("absence with 1 op", _with(one, value=None), "expected 1 arg, got 0"),
        ("absence with 2 ops", _with(two, value=None), "expected 1 arg, got 0"),
        ("absence: the key check comes first", _with(one, value=None, keys=[b"nope"]), "key mismatch on operation #0"),
        ("nil final root (one aunt too few)", _with(one, ops=[_op(one.ops[0], aunts=one.ops[0].proof.aunts[:-1])]),
         "calculated root hash is invalid: expected " + one.root.hex().upper() + " but got "),
        ("nil final root (one aunt too many)", _with(one, ops=[_op(one.ops[0], aunts=one.ops[0].proof.aunts + [h32])]),
         "calculated root hash is invalid: expected "),
        ("nil final root (index = total)", _with(one, ops=[_op(one.ops[0], index=11)]), "calculated root hash is invalid"),
        ("nil final root (total = 0)", _with(one, ops=[_op(one.ops[0], total=0, index=0, aunts=[])]), "calculated root hash is invalid"),
        ("a nil final root equals an empty root", _with(one, ops=[_op(one.ops[0], index=11)], root=b""), None),
        ("an empty root against a computed one", _with(one, root=b""), "calculated root hash is invalid: expected  but got " + one.root.hex().upper()),
        ("a root of 31 bytes", _with(one, root=one.root[:31]), "calculated root hash is invalid: expected " + one.root[:31].hex().upper() + " but got "),
        ("a root of 33 bytes", _with(one, root=one.root + b"\0"), "calculated root hash is invalid: expected " + one.root.hex().upper() + "00 but got "),
        ("an empty op key consumes nothing", _with(one, ops=[_op(one.ops[0], key=b"")], keys=[]), "leaf hash mismatch: want "),
        ("no ops: the value is the root", H.ProofOpsItem([], b"value", [], b"value"), None),
        ("no ops: another root", H.ProofOpsItem([], b"root", [], b"value"), "calculated root hash is invalid: expected 726F6F74 but got 76616C7565"),
        ("no ops: keys left", H.ProofOpsItem([], b"v", [b"k"], b"v"), "keypath not consumed all"),
        ("no ops: empty value and root", H.ProofOpsItem([], b"", [], b""), None),
    ]
    # an op with an empty key whose proof is valid for it: consumes no key, the next op takes the only one
    inner = SM.SimpleMap({b"": b"v0", b"a": b"v1"}, gen)
    outer = SM.SimpleMap({b"sub": inner.root, b"zzz": b"v2"}, gen)
    cases.append(("a valid op with an empty key", H.ProofOpsItem([inner.op(b""), outer.op(b"sub")], outer.root, [b"sub"], b"v0"), None))
    # a malformed middle proof (index >= total): its nil root feeds SHA-256("") to the next op
    empty_outer = SM.SimpleMap({b"bank": b"", b"other": b"v"}, gen)
    bad_mid = _op(o0, index=11)
    cases.append(("a nil middle root is passed on as the empty string",
                  H.ProofOpsItem([bad_mid, empty_outer.op(b"bank")], empty_outer.root, [b"bank", b"bank/key-004"], two.value), None))
    cases.append(("a nil middle root against a real next op", _with(two, ops=[bad_mid, o1]),
                  "leaf hash mismatch: want " + o1.proof.leaf_hash.hex().upper() + " got "
                  + R.ValueOp(b"bank", None).kv_hash(b"").hex().upper()))
    long_key = b"k" * 300  # a text longer than the stride is cut
    cases.append(("a long key", H.ProofOpsItem([H.ValueOp(long_key, one.ops[0].proof)], one.root, [b"q"], b"v"),
                  "key mismatch on operation #0: expected q but got kkkk"))
    _CASES = cases
    return cases


_TX = None


def tx_cases():
    """[(name, host.TxProof, expected text or None)]."""
    global _TX
    if _TX is not None:
        return _TX
    rng = random.Random(21)
    txs = [_bytes(rng, 250 if i else 0) for i in range(13)]  # tx 0 is empty
    root, proofs = P.txs_proofs(txs)
    h32 = _bytes(rng, 32)

    def tx(i, root_hash=root, data_hash=root, data=None, **kw):
        p = proofs[i]
        d = dict(total=p.total, index=p.index, leaf_hash=p.leaf_hash, aunts=list(p.aunts))
        d.update(kw)
        return H.TxProof(root_hash, txs[i] if data is None else data, H.Proof(**d), data_hash)

    bad, inc = "proof matches different data hash", "proof is not internally consistent"
    cases = [("ok tx %d" % i, tx(i), None) for i in range(len(txs))]
    root1, proofs1 = P.txs_proofs(txs[:1])
    cases += [
        ("a block of one tx", H.TxProof(root1, txs[0], H.Proof(1, 0, proofs1[0].leaf_hash, []), root1), None),
        ("another data hash", tx(3, data_hash=h32), bad),
        ("an empty data hash", tx(3, data_hash=b""), bad),
        ("a data hash of 31 bytes", tx(3, data_hash=root[:31]), bad),
        ("data hash first", tx(3, data_hash=h32, index=-1, total=0), bad),
        ("negative index", tx(3, index=-1), "proof index cannot be negative"),
        ("negative index before total", tx(3, index=-1, total=0), "proof index cannot be negative"),
        ("Total == 0", tx(3, total=0), "proof total must be positive"),
        ("negative total", tx(3, total=-5), "proof total must be positive"),
        ("another tx", tx(3, data=txs[4]), inc),
        ("a flipped aunt", tx(3, aunts=[h32] + list(proofs[3].aunts[1:])), inc),
        ("one aunt too few", tx(3, aunts=list(proofs[3].aunts[:-1])), inc),
        ("index = total", tx(3, index=13), inc),
        ("both hashes wrong but equal", tx(3, root_hash=h32, data_hash=h32), inc),
        ("a leaf hash of 31 bytes", tx(3, leaf_hash=proofs[3].leaf_hash[:31]), inc),
        ("an empty leaf hash", tx(3, leaf_hash=b""), inc),
        ("a 33-byte aunt", tx(3, aunts=[proofs[3].aunts[0] + b"\0"] + list(proofs[3].aunts[1:])), inc),
        ("a nil root equals an empty root hash", tx(3, root_hash=b"", data_hash=b"", aunts=[]), None),
        ("an empty root hash against a computed root", tx(3, root_hash=b"", data_hash=b""), inc),
    ]
    # a 33-byte aunt that verifies: innerHash takes any length (no ValidateBasic here)
    a33 = h32 + b"\x07"
    leaf = proofs[3].leaf_hash
    from merkle_ref import inner_hash
    cases.append(("a 33-byte aunt that verifies", H.TxProof(inner_hash(leaf, a33), txs[3], H.Proof(2, 0, leaf, [a33]),
                                                             inner_hash(leaf, a33)), None))
    want = [R.tx_proof_validate(t.root_hash, t.data, P.Proof(t.proof.total, t.proof.index, t.proof.leaf_hash, t.proof.aunts),
                                t.data_hash) for _, t, _ in cases]
    assert want == [w for _, _, w in cases], [(n, a, b) for (n, _, b), a in zip(cases, want) if a != b]
    _TX = cases
    return cases


def check_proof_ops(ctx, lib):
    cases = proof_ops_cases()
    items = [it for _, it, _ in cases]
    want = [expected(it) for it in items]
    for (name, _, start), w in zip(cases, want):  # the restatement against the stated texts
        assert (w is None) if start is None else (w is not None and w.startswith(start[:ERR_CUT])), (name, w)
    got = H.proof_ops_verify(ctx, items, lib=lib)
    assert got == want, [(n, g, w) for (n, _, _), g, w in zip(cases, got, want) if g != w]
    # each alone: the result does not depend on its neighbours
    assert [H.proof_ops_verify(ctx, [it], lib=lib)[0] for it in items[:12]] == want[:12]
    return want


def check_tx_proofs(ctx, lib):
    cases = tx_cases()
    got = H.tx_proofs_validate(ctx, [t for _, t, _ in cases], lib=lib)
    assert got == [w for _, _, w in cases], [(n, g, w) for (n, _, w), g in zip(cases, got) if g != w]


# ---- the golden file (tests/golden/proof_ops_vectors.json)
def _proof_json(p):
    return {"total": p.total, "index": p.index, "leaf_hash": p.leaf_hash.hex(), "aunts": [a.hex() for a in p.aunts]}


def _proof_of(d):
    return H.Proof(d["total"], d["index"], bytes.fromhex(d["leaf_hash"]), [bytes.fromhex(a) for a in d["aunts"]])


def golden_document():
    ops = [{"name": name, "ops": [{"key": op.key.hex(), "proof": _proof_json(op.proof)} for op in it.ops],
            "root": it.root.hex(), "keys": [k.hex() for k in it.keys],
            "value": None if it.value is None else it.value.hex(), "error": expected(it)}
           for name, it, _ in proof_ops_cases()]
    txs = [{"name": name, "root_hash": t.root_hash.hex(), "data": t.data.hex(), "proof": _proof_json(t.proof),
            "data_hash": t.data_hash.hex(), "error": want} for name, t, want in tx_cases()]
    return {"comment": "written by tests/golden/make_proof_ops_golden.py from tests/proof_ops_ref.py; "
                       "unpinned by reference-held vectors", "err_stride": H.ERR_STRIDE, "proof_ops": ops, "tx_proofs": txs}


def load_golden(path):
    doc = json.load(open(path))
    ops = [(d["name"], H.ProofOpsItem([H.ValueOp(bytes.fromhex(o["key"]), _proof_of(o["proof"])) for o in d["ops"]],
                                      bytes.fromhex(d["root"]), [bytes.fromhex(k) for k in d["keys"]],
                                      None if d["value"] is None else bytes.fromhex(d["value"])), d["error"])
           for d in doc["proof_ops"]]
    txs = [(d["name"], H.TxProof(bytes.fromhex(d["root_hash"]), bytes.fromhex(d["data"]), _proof_of(d["proof"]),
                                 bytes.fromhex(d["data_hash"])), d["error"]) for d in doc["tx_proofs"]]
    return ops, txs
