// Commit.Hash on the host (types/block.go:900-918): the protobuf bytes of a
// CommitSig (proto/tendermint/types/types.pb.go:1764-1797) and the merkle
// root over them.  The engine's k_commit_leaves (commit_kernels.hip) encodes
// the same bytes on the device; this is the host layer's fallback and the
// path of commits the engine refuses (flags above 127, addresses that are not
// 0 or 20 bytes, signatures above 64 bytes).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/tmhost.h"
#include "tm_light.h"
#include "tm_types.h"

namespace tmh {

// tmproto.CommitSig.Marshal of s, appended to out.  proto3: zero values are
// omitted; the timestamp (stdtime, non-nullable) is always present, its
// seconds and nanos omitted when zero and in the 10-byte form when negative.
// Seconds outside [-62135596800, 253402300800) and nanos outside [0, 1e9) are
// outside the reference's domain (StdTimeMarshalTo fails); they are encoded as
// plain protobuf.
inline void AppendCommitSigProto(const tmv_commit_sig &s, Bytes &out) {
  uint8_t tmp[48], *p = tmp;  // at most 3 + 6 + 2 + 22 + 6 bytes around the address and the signature
  if (s.block_id_flag) {
    *p++ = 0x08;
    p = PutUvarintP(p, s.block_id_flag);
  }
  if (s.validator_address_len) {
    *p++ = 0x12;
    p = PutUvarintP(p, s.validator_address_len);
    out.insert(out.end(), tmp, p);
    out.insert(out.end(), s.validator_address, s.validator_address + s.validator_address_len);
    p = tmp;
  }
  const uint64_t sec = (uint64_t)s.ts_seconds, nan = (uint64_t)(int64_t)s.ts_nanos;
  *p++ = 0x1a;
  *p++ = (uint8_t)((sec ? 1 + UvarintLen(sec) : 0) + (nan ? 1 + UvarintLen(nan) : 0));
  if (sec) {
    *p++ = 0x08;
    p = PutUvarintP(p, sec);
  }
  if (nan) {
    *p++ = 0x10;
    p = PutUvarintP(p, nan);
  }
  if (s.signature_len) {
    *p++ = 0x22;
    p = PutUvarintP(p, s.signature_len);
  }
  out.insert(out.end(), tmp, p);
  if (s.signature_len) out.insert(out.end(), s.signature, s.signature + s.signature_len);
}

// Commit.Hash of a non-nil commit.
inline void CommitHashHost(const tmv_commit &c, uint8_t out[32]) {
  Bytes blob;
  std::vector<uint32_t> off{0};
  blob.reserve(112ull * c.n_sigs);
  off.reserve(c.n_sigs + 1);
  for (uint32_t i = 0; i < c.n_sigs; i++) {
    AppendCommitSigProto(c.sigs[i], blob);
    off.push_back((uint32_t)blob.size());
  }
  MerkleRootHost(blob.data(), off.data(), c.n_sigs, out);
}

}  // namespace tmh
