"""The host path of tmv_proof_ops_verify and tmv_tx_proofs_validate: the host
layer built without the engine (tests/native/proofops, libproofopshost.so: its
weak references to the engine stay null) against the restatement of the
reference (tests/proof_ops_ref.py) and the golden file written from it.  No GPU."""
import ctypes
import os

import pytest

import proof_ops_cases as C
from tendermint_amd import host as H
from tendermint_amd._native import NativeError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libproofopshost.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "proof_ops_vectors.json")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return ctypes.CDLL(LIB)


def test_proof_ops_sequencing_and_texts(lib):
    want = C.check_proof_ops(None, lib)
    texts = [w for w in want if w]
    for start in ("decoding proof: decoding a proof operator: negative Total",
                  "decoding proof: decoding a proof operator: negative Index",
                  "decoding proof: decoding a proof operator: expected LeafHash size to be 32, got 31",
                  "decoding proof: decoding a proof operator: expected no more than 100 aunts, got 101",
                  "decoding proof: decoding a proof operator: expected Aunts#1 size to be 32, got 5",
                  "key path has insufficient # of parts: expected no more keys but got ",
                  "key mismatch on operation #0: expected ", "key mismatch on operation #1: expected ",
                  "expected 1 arg, got 0", "leaf hash mismatch: want ", "calculated root hash is invalid: expected ",
                  "keypath not consumed all"):
        assert any(t.startswith(start) for t in texts), start
    assert any(t.endswith(" but got ") for t in texts)            # a nil computed root prints as nothing
    assert any(len(t) == C.ERR_CUT for t in texts)                # a text cut to the stride
    assert sum(1 for w in want if w is None) >= 9


def test_tx_proofs_texts(lib):
    C.check_tx_proofs(None, lib)
    texts = {w for _, _, w in C.tx_cases()}
    assert texts == {None, "proof matches different data hash", "proof index cannot be negative",
                     "proof total must be positive", "proof is not internally consistent"}


def test_golden_file(lib):
    ops, txs = C.load_golden(GOLDEN)
    assert len(ops) >= 40 and len(txs) >= 30
    assert H.proof_ops_verify(None, [it for _, it, _ in ops], lib=lib) == [w for _, _, w in ops]
    assert H.tx_proofs_validate(None, [t for _, t, _ in txs], lib=lib) == [w for _, _, w in txs]


def test_golden_file_is_the_generators():
    """The committed file is what tests/golden/make_proof_ops_golden.py writes from the restatement."""
    import json
    assert json.load(open(GOLDEN)) == json.loads(json.dumps(C.golden_document()))


def test_argument_errors_and_empty_calls(lib):
    assert H.proof_ops_verify(None, [], lib=lib) == []
    assert H.tx_proofs_validate(None, [], lib=lib) == []
    with pytest.raises(NativeError, match=r"\(-1\)"):     # no ops and no value: the reference panics
        H.proof_ops_verify(None, [H.ProofOpsItem([], b"root", [], None)], lib=lib)
    ok = C.proof_ops_cases()[0][1]
    with pytest.raises(NativeError, match=r"\(-1\)"):     # one such item fails the call
        H.proof_ops_verify(None, [ok, H.ProofOpsItem([], b"", [b"k"], None)], lib=lib)


def test_threshold_knob_is_harmless_without_the_engine(lib, monkeypatch):
    monkeypatch.setenv("TMV_DEVICE_PROOF_OPS_MIN", "0")
    C.check_proof_ops(None, lib)
    C.check_tx_proofs(None, lib)
