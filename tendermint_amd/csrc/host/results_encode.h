// The hash of a block's ABCI results on the host: the protobuf bytes of the
// deterministic fields of ExecTxResult (abci/types/types.go:213-239,
// types.pb.go:3165-3170) and the merkle root over them, and
// ConsensusParams.HashConsensusParams (types/params.go:385-399).  The engine's
// k_result_leaves (results_kernels.hip) encodes the same bytes on the device;
// this is the host layer's fallback and the path of trees with a long result.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/tmhost.h"
#include "tm_light.h"
#include "tm_types.h"

namespace tmh {

// The bytes around a result's data: [08 uvarint(code)] [12 uvarint(L)] into
// head (at most 12 bytes), [28 varint(gas_wanted)] [30 varint(gas_used)] into
// tail (at most 22).  proto3: zero and empty fields are omitted; a negative
// int64 is the 10-byte two's-complement varint.  Returns the head's length,
// *tail_len the tail's.
inline size_t TxResultFrame(const tmv_tx_result &r, uint8_t head[12], uint8_t tail[22], size_t *tail_len) {
  uint8_t *p = head;
  if (r.code) {
    *p++ = 0x08;
    p = PutUvarintP(p, r.code);
  }
  if (r.data.len) {
    *p++ = 0x12;
    p = PutUvarintP(p, r.data.len);
  }
  uint8_t *t = tail;
  if (r.gas_wanted) {
    *t++ = 0x28;
    t = PutUvarintP(t, (uint64_t)r.gas_wanted);
  }
  if (r.gas_used) {
    *t++ = 0x30;
    t = PutUvarintP(t, (uint64_t)r.gas_used);
  }
  *tail_len = (size_t)(t - tail);
  return (size_t)(p - head);
}

// ExecTxResult.Marshal of r's deterministic fields, appended to out.
inline void AppendTxResultProto(const tmv_tx_result &r, Bytes &out) {
  uint8_t head[12], tail[22];
  size_t tl;
  const size_t hl = TxResultFrame(r, head, tail, &tl);
  out.insert(out.end(), head, head + hl);
  if (r.data.len) out.insert(out.end(), r.data.p, r.data.p + r.data.len);
  out.insert(out.end(), tail, tail + tl);
}

// merkle.HashFromByteSlices over MarshalTxResults(rs), behind the leading
// leaf *first when it is not null.
inline void TxResultsRootHost(const tmv_tx_result *rs, uint32_t n, const tmv_bytes *first, uint8_t out[32]) {
  static const uint8_t zero = 0;
  const size_t lead = first ? 1 : 0, leaves = lead + n;
  Digest root;
  if (leaves == 0) {
    Sha256Bytes(root.w, nullptr, 0, nullptr, 0);  // emptyHash()
  } else {
    std::vector<Digest> lv(leaves);
    if (first) Sha256Bytes(lv[0].w, &zero, 1, first->p, first->len);
    Bytes leaf;
    for (uint32_t i = 0; i < n; i++) {
      leaf.clear();
      AppendTxResultProto(rs[i], leaf);
      Sha256Bytes(lv[lead + i].w, &zero, 1, leaf.data(), leaf.size());
    }
    root = MerkleRootHostRange(lv.data(), leaves);
  }
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(root.w[i] >> (24 - 8 * b));
}

// SHA-256 of tmproto.HashedParams{BlockMaxBytes, BlockMaxGas}.Marshal().
inline void ConsensusParamsHashHost(int64_t block_max_bytes, int64_t block_max_gas, uint8_t out[32]) {
  uint8_t buf[22], *p = buf;
  if (block_max_bytes) {
    *p++ = 0x08;
    p = PutUvarintP(p, (uint64_t)block_max_bytes);
  }
  if (block_max_gas) {
    *p++ = 0x10;
    p = PutUvarintP(p, (uint64_t)block_max_gas);
  }
  Digest d;
  Sha256Bytes(d.w, nullptr, 0, buf, (size_t)(p - buf));
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(d.w[i] >> (24 - 8 * b));
}

}  // namespace tmh
