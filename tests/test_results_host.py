"""The tx-result encoder, the results roots, HashConsensusParams, the light
client's BlockResults / ConsensusParams checks and blocksync_replay_stateful on
the CPU: the host layer built without the engine (tests/native/results,
libresultshost.so: its weak references to the engine stay null) against the
restatement of the reference (tests/results_ref.py).  The GPU twin is
tests/test_gpu_results.py."""
import ctypes
import json
import os
import subprocess

import pytest

import merkle_ref as M
import results_cases as C
import results_ref as R
from tendermint_amd import chains, host as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libresultshost.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "tx_results_vectors.json")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    L.rs_tx_result_encode.restype = ctypes.c_size_t
    L.rs_tx_result_encode.argtypes = [ctypes.POINTER(H.CTxResult), ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t]
    return L


def _encode(lib, code, data, gas_wanted, gas_used) -> bytes:
    k = H._Keep()
    arr = H._c_tx_results(k, [H.TxResult(code, data, gas_wanted, gas_used)])
    out = (ctypes.c_uint8 * 20000)()
    n = lib.rs_tx_result_encode(arr, out, 20000)
    return bytes(out[:n])


def test_restatement_reproduces_the_literal_encodings(lib):
    """The hand-derived encodings pin the restatement; the product's encoder gives the same bytes."""
    for v in json.load(open(GOLDEN))["encodings"]:
        data = bytes.fromhex(v["data_hex"]) if v["data_hex"] is not None else b""
        case = (v["code"], data, v["gas_wanted"], v["gas_used"])
        assert R.tx_result_bytes(*case).hex() == v["enc_hex"]
        assert _encode(lib, *case).hex() == v["enc_hex"]


def test_case_lengths():
    C.check_case_lengths()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_encoder_bytes(lib, name):
    case = C.CASES[name]
    assert _encode(lib, *case) == R.tx_result_bytes(*case)


@pytest.mark.parametrize("first", [False, True])
def test_results_roots_host(lib, first):
    trees = [C.tree(n, 10 + n) for n in C.TREE_SIZES] + [list(C.CASES.values())]
    firsts = [C._data(0 if k % 3 == 0 else 40 * k) for k in range(len(trees))] if first else None
    got = H.results_hashes(None, [C.host_results(t) for t in trees], firsts, lib)
    assert got == [R.results_hash(t, firsts[k] if first else None) for k, t in enumerate(trees)]
    if not first:
        assert got[0] == M.empty_hash()
        assert got[1] == M.leaf_hash(R.tx_result_bytes(*trees[1][0]))
    else:
        assert got[0] == M.leaf_hash(b"")  # no results behind an empty leading leaf: one leaf, not the empty tree
    assert H.results_hashes(None, [], None, lib) == []


def test_results_roots_one_at_a_time_equal_the_batch(lib):
    trees = [C.host_results(C.tree(n, 50 + n)) for n in (0, 1, 5, 65)]
    assert [H.results_hashes(None, [t], None, lib)[0] for t in trees] == H.results_hashes(None, trees, None, lib)


@pytest.mark.parametrize("params", [(0, 0), (22020096, -1), (1, 1), (C.I64_MAX, C.I64_MIN)])
def test_consensus_params_hash(lib, params):
    assert H.consensus_params_hash(*params, lib=lib) == R.consensus_params_hash(*params)
    if params == (0, 0):
        assert H.consensus_params_hash(0, 0, lib=lib) == M.empty_hash()


def test_block_results_verify(lib):
    items = C.block_results_items()
    want = [w for _, w in items]
    assert want.count(None) == 6 and want.count(R.HEIGHT_TEXT) == 2
    assert sum(w is not None and w.startswith("last results ") for w in want) == 4
    assert H.block_results_verify(None, [it for it, _ in items], lib) == want
    assert H.block_results_verify(None, [], lib) == []


def test_consensus_params_verify(lib):
    items = C.consensus_params_items()
    want = [w for _, w in items]
    assert want.count(None) == 4 and want.count(R.HEIGHT_TEXT) == 2
    assert sum(w is not None and w.startswith("params hash ") for w in want) == 3
    assert H.consensus_params_verify(None, [it for it, _ in items], lib) == want
    assert H.consensus_params_verify(None, [], lib) == []


def test_argument_errors(lib):
    H._setup_results(lib)
    out = (ctypes.c_uint8 * 64)()
    outp = ctypes.cast(out, H._u8p)
    counts = (ctypes.c_uint32 * 2)(1, 0)
    ptrs = (ctypes.POINTER(H.CTxResult) * 2)()
    res = (ctypes.c_int32 * 2)()
    assert lib.tmv_results_hash_many(None, None, counts, None, 1, outp) < 0
    assert lib.tmv_results_hash_many(None, ptrs, None, None, 1, outp) < 0
    assert lib.tmv_results_hash_many(None, ptrs, counts, None, 1, None) < 0
    assert lib.tmv_results_hash_many(None, ptrs, counts, None, 1, outp) < 0            # one result, null list
    bad = (H.CTxResult * 1)(H.CTxResult(0, H.CBytes(None, 3), 0, 0))                   # data length without data
    ptrs[0] = ctypes.cast(bad, ctypes.POINTER(H.CTxResult))
    assert lib.tmv_results_hash_many(None, ptrs, counts, None, 1, outp) < 0
    bad[0] = H.CTxResult(0, H.CBytes(None, 0), 0, 0)
    firsts = (H.CBytes * 1)(H.CBytes(None, 2))                                          # a leading leaf likewise
    assert lib.tmv_results_hash_many(None, ptrs, counts, firsts, 1, outp) < 0
    assert lib.tmv_results_hash_many(None, ptrs, counts, None, 1, outp) == 0
    assert lib.tmv_results_hash_many(None, None, None, None, 0, None) == 0
    assert lib.tmv_consensus_params_hash(1, 1, None) < 0
    assert lib.tmv_block_results_verify(None, None, 1, res, None, 0) < 0
    assert lib.tmv_consensus_params_verify(None, None, 1, res, None, 0) < 0
    item = (H.CBlockResultsIn * 1)(H.CBlockResultsIn(1, None, 1, H.CBytes(None, 0), H.CBytes(None, 0)))
    assert lib.tmv_block_results_verify(None, item, 1, res, None, 0) < 0               # one result, null list
    assert lib.tmv_block_results_verify(None, item, 1, None, None, 0) < 0
    par = (H.CConsensusParamsIn * 1)(H.CConsensusParamsIn(1, 1, 1, H.CBytes(None, 32)))
    assert lib.tmv_consensus_params_verify(None, par, 1, res, None, 0) < 0


def test_go_time_string():
    assert chains.go_time_string((0, 0)) == "1970-01-01 00:00:00 +0000 UTC"
    assert chains.go_time_string((-62135596800, 0)) == "0001-01-01 00:00:00 +0000 UTC"
    assert chains.go_time_string((1577836800, 999999999)) == "2020-01-01 00:00:00.999999999 +0000 UTC"
    assert chains.go_time_string((1577836799, 1000)) == "2019-12-31 23:59:59.000001 +0000 UTC"


def test_evidence_byte_size():
    assert chains.evidence_byte_size([]) == 0
    assert chains.evidence_byte_size([b""]) == 2
    assert chains.evidence_byte_size([b"a" * 127, b"b" * 128]) == (1 + 1 + 127) + (1 + 2 + 128)
    assert chains.evidence_byte_size(C.EVIDENCE) == 177


@pytest.fixture(scope="module")
def scenarios():
    return C.replay_scenarios()


@pytest.fixture(scope="module")
def fake():
    import commit_fixtures as F
    fb = F.FakeBackend()
    fb.real_signatures(True)
    yield fb
    fb.real_signatures(False)


@pytest.mark.parametrize("window,depth", [(1, 1), (5, 2), (100, 1)])
def test_blocksync_replay_stateful(lib, fake, scenarios, window, depth):
    import commit_fixtures as F

    def run(state, blocks, records):
        vh = M.validator_set_hash([(v.pub_key, v.key_kind, v.voting_power) for v in state.validators.validators])
        return chains.blocksync_replay_stateful(None, state, blocks, records, window=window, depth=depth,
                                                part_size=128, lib=lib, vals_hash=vh,
                                                verify_commits=lambda jobs: F.fake_verify_commits(fake, jobs))
    C.check_replay(run, scenarios)


def test_stateful_chain_is_the_full_chain_with_real_app_hashes(lib):
    """The generator's option changes the three hashes alone, and the honest
    chain still replays clean through blocksync_replay_full."""
    from tendermint_amd.testing.blocks import make_full_chain
    state, blocks, ids, records = C.stateful_chain()
    vals, plain, _ = make_full_chain(C.N_BLOCKS, C.N_VALS, C.CHAIN, seed=41, raw_len=(1, 300), part_size=128, txs=(1, 4))
    assert vals == state.validators and len(records) == len(blocks)
    for a, b, r in zip(blocks, plain, records):
        assert (a.txs, a.evidence, a.raw, a.header.data_hash) == (b.txs, b.evidence, b.raw, b.header.data_hash)
        assert len(r.results) == len(a.txs)
    assert blocks[0].header.last_results_hash == M.empty_hash()
    assert blocks[3].header.last_results_hash == R.results_hash(C.as_tuples(records[2].results))
    assert blocks[3].header.app_hash == records[2].app_hash
    assert blocks[3].header.consensus_hash == R.consensus_params_hash(22020096, -1)


def test_replay_needs_a_record_per_applied_block(lib, scenarios):
    state, blocks, records, _ = scenarios["clean"]
    with pytest.raises(ValueError, match="records"):
        chains.blocksync_replay_stateful(None, state, blocks, records[:5], verify_commits=lambda jobs: [], lib=lib,
                                         vals_hash=b"")


def test_results_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "results"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "results_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
