"""Block part sets and proof verification through the host layer on the device
path (include/tmhost.h over tmv_merkle_proofs / tmv_merkle_verify_proofs):
the host / device threshold is set to 0 for these calls, so every one of them
reaches the engine.  The same cases as the CPU test of the host fallback."""
import pytest

import merkle_host_cases as C
from tendermint_amd import host as H

pytestmark = pytest.mark.gpu


@pytest.fixture()
def device_path(monkeypatch):
    monkeypatch.setenv("TMV_DEVICE_MERKLE_MIN", "0")


@pytest.mark.parametrize("part_size", [C.PART, 4096])
def test_part_sets_on_the_device(ctx, device_path, part_size):
    ctx.kernel_timing(True)
    try:
        for k in ("k_merkle_tree_levels", "k_merkle_verify_proofs"):
            ctx.kernel_timing_read(k)
        C.check_part_sets(ctx, None, part_size)
        # the calls did reach the engine
        assert ctx.kernel_timing_read("k_merkle_tree_levels")[1] >= 2
        assert ctx.kernel_timing_read("k_merkle_verify_proofs")[1] >= 1
    finally:
        ctx.kernel_timing(False)


@pytest.mark.parametrize("big", [False, True], ids=["short", "parts"])
def test_proofs_verify_on_the_device(ctx, device_path, big):
    C.check_proofs_verify(ctx, None, big=big)


def test_default_threshold_keeps_small_calls_on_the_host(ctx, monkeypatch):
    monkeypatch.delenv("TMV_DEVICE_MERKLE_MIN", raising=False)
    ctx.kernel_timing(True)
    try:
        ctx.kernel_timing_read("k_merkle_tree_levels")
        C.check_part_sets(ctx, None, C.PART)
        assert ctx.kernel_timing_read("k_merkle_tree_levels")[1] == 0
    finally:
        ctx.kernel_timing(False)
