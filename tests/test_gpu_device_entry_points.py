"""The four device-pointer entry points share what they do before a launch
(DeviceCall in csrc/tmverify_runtime.cpp), and two of them are special cases of
tmv_verify_batch_device_ex: on one context, the same device-resident batch
through each gives the same status vector and TMV_NOT_ALL, and a device that is
not in the context is refused by each with the same code and text."""
import numpy as np
import pytest

import oracle_c as C
from tendermint_amd import _native as N
from tendermint_amd.testing._openssl import Ed25519Signer
from tendermint_amd.testing.factory import Batch, key_seed

pytestmark = pytest.mark.gpu

BAD = 57


def _batch(n=100):
    signers = [Ed25519Signer(key_seed(k, "dev entry")) for k in range(7)]
    ents = []
    for i in range(n):
        msg = b"device entry %d" % i * (1 + i % 3)
        sig = signers[i % 7].sign(msg)
        if i == BAD:
            sig = sig[:40] + bytes([sig[40] ^ 2]) + sig[41:]
        ents.append((signers[i % 7].public_key, msg, sig))
    return Batch.from_entries(ents)


def test_four_entry_points_one_batch(ctx):
    """`ctx` only orders this test after the session's context; the calls share a context of their own."""
    import torch
    dev = torch.device("cuda:0")
    b = _batch()
    _, ref = C.ed25519_verify_packed(b.pk, b.sig, b.msg, b.off, threads=4)
    assert ref.sum() == b.n - 1 and ref[BAD] == 0
    pk, sig, msg = (torch.from_numpy(a).to(dev) for a in (b.pk, b.sig, b.msg))
    off = torch.from_numpy(b.off.view(np.int32)).to(dev)
    kind = torch.zeros(b.n, dtype=torch.uint8, device=dev)  # TMV_KIND_ED25519 on every entry
    outs = {k: torch.full((b.n,), -7, dtype=torch.int8, device=dev) for k in ("ed25519", "mixed", "ex", "batches")}
    p = {k: v.data_ptr() for k, v in outs.items()}
    args = (pk.data_ptr(), sig.data_ptr(), msg.data_ptr(), off.data_ptr(), b.n)
    ref1 = N.BatchRef(pk.data_ptr(), sig.data_ptr(), msg.data_ptr(), off.data_ptr(), b.n, len(b.msg), 0)
    stream = torch.cuda.current_stream().cuda_stream
    own = N.Context(1)
    L, h = own._lib, own._h

    def calls(device):
        refs = (N.BatchRef * 1)(ref1)
        refs[0].status = p["batches"]
        return {
            "ed25519": L.tmv_ed25519_verify_batch_device(h, device, *args, p["ed25519"], stream),
            "mixed": L.tmv_verify_mixed_batch_device(h, device, kind.data_ptr(), *args, p["mixed"], stream),
            "ex": L.tmv_verify_batch_device_ex(h, device, N.TMV_KIND_ED25519, 0, None, *args, p["ex"], stream),
            "batches": L.tmv_verify_batches_device(h, device, N.TMV_KIND_ED25519, 0, refs, 1, stream),
        }

    try:
        torch.cuda.synchronize()
        # a device that is not in the context: refused before anything is launched
        for device in (1 << 20, -1):
            for name in outs:
                rc = calls(device)[name]
                assert rc == N.TMV_ERR_ARG and N.last_error() == "device not in context", name
        # the kinds are checked by _ex alone, behind the device and the empty batch
        assert L.tmv_verify_batch_device_ex(h, 0, N.TMV_KIND_MIXED, 0, None, *args, p["ex"], stream) == N.TMV_ERR_ARG
        assert N.last_error() == "mixed batch without kinds"
        assert L.tmv_verify_batch_device_ex(h, 0, N.TMV_KIND_MIXED + 1, 0, None, *args, p["ex"], stream) == N.TMV_ERR_ARG
        assert N.last_error() == "unsupported key kind"
        assert L.tmv_verify_batch_device_ex(h, 0, N.TMV_KIND_MIXED, 0, None, *args[:4], 0, p["ex"], stream) == N.TMV_NOT_ALL
        torch.cuda.synchronize()
        assert all((o.cpu().numpy() == -7).all() for o in outs.values())
        assert calls(0) == {name: N.TMV_NOT_ALL for name in outs}
        torch.cuda.synchronize()
        for name, o in outs.items():
            assert np.array_equal(o.cpu().numpy().view(np.uint8), ref), name
    finally:
        torch.cuda.synchronize()
        own.close()
