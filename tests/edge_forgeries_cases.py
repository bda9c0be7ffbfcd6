"""tests/golden/edge_forgeries.json for the CPU and GPU tests: the records of
one scheme as entries with their expected statuses, and the BatchVerifier case
both backends run (one rejected sr25519 key of every class between two honest
entries)."""
import numpy as np

# the Ristretto rejection classes of the fixture's key_identity/... and r_identity/... records
SR_CLASSES = ("negative", "nonsquare_flipped_i", "nonsquare_none", "neg_t", "y_zero", "noncanonical", "bit255")


def records(golden, scheme=None):
    vs = golden("edge_forgeries.json")["vectors"]
    return [v for v in vs if scheme is None or v["scheme"] == scheme]


def entry(v):
    return bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])


def entries(vs):
    return [entry(v) for v in vs]


def statuses(vs):
    return np.array([v["status"] for v in vs], np.int8)


def name_parts(v):
    return v["name"].split("/")


def rejected_key_per_class(golden):
    """{class: (pk, msg, sig)}: of every class one key_identity record with s = 1, whose
    R = [1]B verifies under a key that acts as the identity."""
    out = {}
    for v in records(golden, "sr25519"):
        p = name_parts(v)
        if p[0] == "key_identity" and p[3] == "s=1":
            out.setdefault(p[1], entry(v))
    assert set(out) == set(SR_CLASSES)
    return out


def check_batch_verifier_rejected_keys(backend, golden):
    """crypto/sr25519/batch.go:30-33 through the host layer: a key of every
    rejection class at index 1 of 3 is the deferred Add error of that index,
    and the entries around it stay valid."""
    from tendermint_amd import host as H
    from tendermint_amd.testing.sr25519_factory import Sr25519Signer
    SR = H.TMV_KIND_SR25519
    priv = Sr25519Signer(bytes([77]) * 32)
    msg = b"edge forgeries"
    sig = priv.sign(msg, b"n")
    for cls, bad in rejected_key_per_class(golden).items():
        v = backend.new(SR)
        for pk, m, s in ((priv.public_key, msg, sig), bad, (priv.public_key, msg, sig)):
            assert v.add(SR, pk, m, s) is None
        ok, valid = v.verify()
        assert not ok and valid == [True, False, True], cls
        idx, text = v.deferred_add_error
        assert idx == 1 and text.startswith("sr25519: invalid public key: "), (cls, idx, text)
