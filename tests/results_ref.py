"""CPU restatement of what the results layer computes (TEST INFRASTRUCTURE: the
checker for tmv_tx_results_hashes, tmv_results_hash_many,
tmv_consensus_params_hash, tmv_block_results_verify and
tmv_consensus_params_verify; never imported by the product path).

Follows, in the reference:
  proto/tendermint/abci/types.proto             ExecTxResult: code = 1 (uint32), data = 2 (bytes),
                                                gas_wanted = 5 (int64), gas_used = 6 (int64)
  abci/types/types.go:213-239                   deterministicExecTxResult, MarshalTxResults
  internal/state/execution.go:262-267           LastResultsHash: no leading leaf
  light/rpc/client.go:439-470                   BlockResults: one leading leaf
  light/rpc/client.go:274-288                   ConsensusParams
  proto/tendermint/types/params.proto           HashedParams: block_max_bytes = 1, block_max_gas = 2 (int64)
  types/params.go:385-399                       HashConsensusParams
hashlib and oracle/merkle_ref.py only; never the product's encoder.
"""
import hashlib

import merkle_ref as M

U64 = (1 << 64) - 1


def uvarint(u: int) -> bytes:
    """Protobuf base-128 varint of u mod 2^64 (an int64 below zero takes 10 bytes)."""
    return M._varint(u & U64)


def _key(field: int, wire: int) -> bytes:
    return uvarint((field << 3) | wire)


def tx_result_bytes(code: int, data: bytes, gas_wanted: int, gas_used: int) -> bytes:
    """ExecTxResult{Code, Data, GasWanted, GasUsed}.Marshal(): proto3 omits
    zero scalars and empty bytes; fields in number order."""
    out = b""
    if code:
        out += _key(1, 0) + uvarint(code)
    if data:
        out += _key(2, 2) + uvarint(len(data)) + data
    if gas_wanted:
        out += _key(5, 0) + uvarint(gas_wanted)
    if gas_used:
        out += _key(6, 0) + uvarint(gas_used)
    return out


def results_hash(results, first=None) -> bytes:
    """merkle.HashFromByteSlices over MarshalTxResults(results), results =
    [(code, data, gas_wanted, gas_used)]; first (bytes, may be empty): the
    light client's leading leaf."""
    leaves = [tx_result_bytes(*r) for r in results]
    if first is not None:
        leaves = [first] + leaves
    return M.hash_from_byte_slices(leaves)


def consensus_params_hash(block_max_bytes: int, block_max_gas: int) -> bytes:
    bz = b""
    if block_max_bytes:
        bz += _key(1, 0) + uvarint(block_max_bytes)
    if block_max_gas:
        bz += _key(2, 0) + uvarint(block_max_gas)
    return hashlib.sha256(bz).digest()


HEIGHT_TEXT = "height must be greater than zero"  # rpc/coretypes/responses.go:20


def block_results_verify(height, results, events, trusted):
    """Client.BlockResults after the fetch: the error text or None."""
    if height <= 0:
        return HEIGHT_TEXT
    mh = results_hash(results, events)
    if mh != trusted:
        return "last results %s does not match with trusted last results %s" % (mh.hex().upper(), trusted.hex().upper())
    return None


def consensus_params_verify(height, block_max_bytes, block_max_gas, trusted):
    """Client.ConsensusParams' last two checks: the error text or None."""
    if height <= 0:
        return HEIGHT_TEXT
    ch = consensus_params_hash(block_max_bytes, block_max_gas)
    if ch != trusted:
        return "params hash %s does not match trusted hash %s" % (ch.hex().upper(), trusted.hex().upper())
    return None
