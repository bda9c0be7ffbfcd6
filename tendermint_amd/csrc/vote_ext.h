// Vote-extension sign-bytes from a per-(chain_id, height, round) template
// (tmv_verify_votes_and_extensions).  VoteExtensionSignBytes
// (types/vote.go:159-172) marshals CanonicalVoteExtension{extension, height,
// round, chain_id} (types/canonical.go:68-78,
// proto/tendermint/types/canonical.pb.go:657-689) length-delimited:
//   M    = uvarint(len(body)) || body
//   body = [0x0a uvarint(E) ext] || tail
//   tail = [0x11 le64(height)] [0x19 le64(round)] [0x22 uvarint(C) chain_id]
// (proto3 omits zero fields).  The precommits of one (chain_id, height, round)
// share the tail: it is the template.  The same length functions size the
// messages on the host (offsets) and on the device (k_vote_ext_signbytes),
// so the two cannot disagree.
#pragma once
#include <cstdint>
#include "votes.h"

namespace tmv {

// Device copy of an extension template: a byte range of the template blob.
struct VoteExtTab {
  uint32_t tail_at, tail_len;
};

// Payloads of at least this many bytes are copied by the whole wave
// (k_vote_ext_signbytes); shorter ones by their own lane.  Measured
// (profiles/vote_ext/bench.json, 100,000 equal payloads per launch): the wave
// copy is slower up to 64 bytes and faster from 96 bytes on.
// TMV_VOTE_EXT_WAVE_MIN overrides it (0 = every payload by its lane).
constexpr uint32_t kVoteExtWaveMin = 96;

// Bytes before the payload: 0x0a uvarint(E), or nothing for an empty one.
TMV_HD uint32_t vote_ext_field_head(uint32_t ext_len) { return ext_len ? 1 + uvarint_len(ext_len) : 0; }

TMV_HD uint32_t vote_ext_body_len(uint32_t tail_len, uint32_t ext_len) {
  return vote_ext_field_head(ext_len) + ext_len + tail_len;
}

TMV_HD uint32_t vote_ext_msg_len(uint32_t tail_len, uint32_t ext_len) {
  const uint32_t body = vote_ext_body_len(tail_len, ext_len);
  return uvarint_len(body) + body;
}

}  // namespace tmv
