// types.VoteExtensionSignBytes (types/vote.go:159-172) on the host:
// MarshalDelimited(CanonicalVoteExtension{extension, height, round,
// chain_id}), field by field as gogoproto emits it
// (proto/tendermint/types/canonical.pb.go:657-689; proto3: zero / empty
// fields omitted):
//   M    = uvarint(len(body)) || body
//   body = [0x0a uvarint(E) ext] || tail
//   tail = [0x11 le64(height)] [0x19 le64(round)] [0x22 uvarint(C) chain_id]
// tail is what the precommits of one (chain_id, height, round) share: the
// template of tmv_verify_votes_and_extensions.  The host encoder and the
// device one (k_vote_ext_signbytes) assemble the same pieces.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "tm_types.h"

namespace tmh {

inline size_t VoteExtTailLen(const std::string &chain_id, int64_t height, int32_t round) {
  return (height != 0 ? 9 : 0) + (round != 0 ? 9 : 0) +
         (chain_id.empty() ? 0 : 1 + UvarintLen(chain_id.size()) + chain_id.size());
}
inline uint8_t *PutVoteExtTail(uint8_t *p, const std::string &chain_id, int64_t height, int32_t round) {
  if (height != 0) { *p++ = 0x11; p = PutFixed64P(p, height); }
  if (round != 0) { *p++ = 0x19; p = PutFixed64P(p, (int64_t)round); }
  if (!chain_id.empty()) {
    *p++ = 0x22;
    p = PutUvarintP(p, chain_id.size());
    std::memcpy(p, chain_id.data(), chain_id.size());
    p += chain_id.size();
  }
  return p;
}
inline Bytes EncodeVoteExtTail(const std::string &chain_id, int64_t height, int32_t round) {
  Bytes t(VoteExtTailLen(chain_id, height, round));
  PutVoteExtTail(t.data(), chain_id, height, round);
  return t;
}

inline size_t VoteExtMsgLen(size_t tail_len, size_t ext_len) {
  const size_t body = (ext_len ? 1 + UvarintLen(ext_len) + ext_len : 0) + tail_len;
  return UvarintLen(body) + body;
}

// One extension's sign-bytes from its template (the host twin of
// k_vote_ext_signbytes), appended to out.
inline void AppendVoteExtFromTail(Bytes &out, const uint8_t *tail, size_t tail_len, const uint8_t *ext,
                                  size_t ext_len) {
  const size_t body = (ext_len ? 1 + UvarintLen(ext_len) + ext_len : 0) + tail_len;
  const size_t at = out.size();
  out.resize(at + UvarintLen(body) + body);
  uint8_t *p = PutUvarintP(out.data() + at, body);
  if (ext_len) {
    *p++ = 0x0a;
    p = PutUvarintP(p, ext_len);
    std::memcpy(p, ext, ext_len);
    p += ext_len;
  }
  if (tail_len) std::memcpy(p, tail, tail_len);
}

inline void AppendVoteExtSignBytes(Bytes &out, const std::string &chain_id, int64_t height, int32_t round,
                                   const uint8_t *ext, size_t ext_len) {
  const Bytes tail = EncodeVoteExtTail(chain_id, height, round);
  AppendVoteExtFromTail(out, tail.data(), tail.size(), ext, ext_len);
}

}  // namespace tmh
