// A strict scanner for the protobuf bytes of a tendermint.types.LightBlock
// (proto/tendermint/types/{types,validator}.proto, crypto/keys.proto): one
// pass, no payload copied.  Host only; needs no engine.  The header and the
// commit are block_wire.h's scanners; this file adds LightBlock, SignedHeader,
// ValidatorSet, Validator and PublicKey.
//
// Canonical is what block_wire.h says, with one difference: a oneof member is
// written even when it is empty, so inside PublicKey the zero-absent rule does
// not apply.  LightBlock.signed_header / validator_set, SignedHeader.header /
// commit and ValidatorSet.proposer are pointers in the reference: absent is
// nil, present with length 0 is non-nil and empty, and the scan keeps the two
// apart (has_*).  Validator.pub_key is nullable = false: always present.
// Handed back besides what block_wire.h hands back -- everything for which
// LightBlockFromProto (types/light.go:104-128) fails without it being a
// ValidateBasic failure, or panics:
//   kKey       a PublicKey with no oneof member, or a key that is not 32 / 33 /
//              32 bytes (crypto/encoding/codec.go:49-78)
//   kProposer  a validator set without proposer (ValidatorFromProto(nil)), or
//              a proposer whose message bytes equal no entry of a non-empty
//              `validators` (the view carries the proposer's index)
//   kPower     the clipped running sum of the voting powers exceeds
//              MaxTotalVotingPower (types/validator_set.go:295-309 panics)
// The first problem in byte order is the one reported -- byte order, not the
// reference's order: LightBlockFromProto decodes every key, then the proposer,
// then sums the powers, so of two faults in one set it may name the other one.
// Either way the block is handed back and nothing is decided.  Nothing outside
// [lo, hi) is read.
//
// Per handled light block: tmv_signed_header / tmv_validator_set views whose
// byte fields point into the caller's bytes, Header.Hash's 14 span leaves
// (block_wire.h) and one tmv_val_span per validator: ValidatorSet.Hash's leaf
// SimpleValidator{pub_key = 1, voting_power = 2} is the Validator message's
// `12 LL <PublicKey> [18 <varint>]` with the two tags replaced
// (include/tmverify.h, tmv_merkle_wire_roots).
#pragma once
#include "block_wire.h"

#pragma GCC visibility push(hidden)
namespace tmw {

constexpr int64_t kMaxTotalVotingPower = INT64_MAX / 8;  // types/validator_set.go:25

struct LightScan {
  BlockScan b;  // the header (b.blk.header, b.hdr_leaf, b.chain_id) and the commit (b.commit, b.sigs)
  bool has_signed_header = false, has_header = false, has_vals = false;
  tmv_signed_header sh{};
  tmv_validator_set vs{};
  std::vector<tmv_validator> vals;
  std::vector<tmv_val_span> val_leaf;  // one per validator, in set order
};

namespace detail {

constexpr Spec kLightBlock{2, 0, bit(1) | bit(2), 0, 0};  // SignedHeader has the same shape
constexpr Spec kValidatorSet{3, bit(3), bit(1) | bit(2), bit(1), bit(2)};  // "required": see scan_validator_set
constexpr Spec kValidator{4, bit(3) | bit(4), bit(2), 0, bit(2)};
constexpr Spec kPublicKey{3, 0, bit(1) | bit(2) | bit(3), 0, 0};  // the oneof: an empty member is written

inline Reason scan_public_key(const uint8_t *d, uint32_t lo, uint32_t hi, tmv_validator *o) {
  Msg m(d, lo, hi, kPublicKey);
  Field f;
  bool more;
  Reason r = m.next(&f, &more);
  if (r != kNone) return r;
  if (!more) return kKey;  // no member: PubKeyFromProto's default case
  static const uint8_t kind[3] = {TMV_KIND_ED25519, TMV_KIND_SECP256K1, TMV_KIND_SR25519};
  o->key_kind = kind[f.num - 1];
  o->pub_key = d + f.pos;
  o->pub_key_len = f.len;
  const Field key = f;
  if ((r = m.next(&f, &more)) != kNone) return r;
  if (more) return kOrder;  // a second member: Marshal writes one
  if (key.len != (key.num == 2 ? 33u : 32u)) return kKey;
  return kNone;
}

// One Validator message.  *leaf: the span of pub_key and voting_power.
inline Reason scan_validator(const uint8_t *d, uint32_t lo, uint32_t hi, tmv_validator *o, tmv_val_span *leaf) {
  *o = tmv_validator{};
  Msg m(d, lo, hi, kValidator);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    switch (f.num) {
      case 1:
        o->address = d + f.pos;
        o->address_len = f.len;
        break;
      case 2:
        if ((r = scan_public_key(d, f.pos, f.pos + f.len, o)) != kNone) return r;
        // the tag is one byte in front of the length; without a power the span ends with the key
        *leaf = tmv_val_span{f.at - 1, f.pos + f.len - (f.at - 1), f.pos + f.len - (f.at - 1)};
        break;
      case 3:
        o->voting_power = (int64_t)f.val;
        leaf->len = m.p - leaf->pos;  // power_at stays where the key ended: the 18
        break;
      default:
        o->proposer_priority = (int64_t)f.val;
    }
  }
}

inline int64_t safe_add_clip(int64_t a, int64_t b) {  // types/validator_set.go:888-897
  int64_t c;
  if (__builtin_add_overflow(a, b, &c)) return b < 0 ? INT64_MIN : INT64_MAX;
  return c;
}

inline Reason scan_validator_set(const uint8_t *d, uint32_t lo, uint32_t hi, LightScan &o) {
  Msg m(d, lo, hi, kValidatorSet);
  Field f;
  bool more;
  int64_t sum = 0;
  std::vector<Field> entry;  // where each `validators` entry lies, for the proposer's comparison
  o.vs.proposer_index = -1;
  for (;;) {
    Reason r = m.next(&f, &more);
    // this message's one required field is the proposer: ValidatorFromProto(nil)
    if (r != kNone) return r == kMissing ? kProposer : r;
    if (!more) return kNone;
    if (f.num == 1) {
      tmv_validator v;
      tmv_val_span leaf{};
      if ((r = scan_validator(d, f.pos, f.pos + f.len, &v, &leaf)) != kNone) return r;
      if ((sum = safe_add_clip(sum, v.voting_power)) > kMaxTotalVotingPower) return kPower;
      o.vals.push_back(v);
      o.val_leaf.push_back(leaf);
      entry.push_back(f);
    } else if (f.num == 2) {
      tmv_validator v;
      tmv_val_span leaf{};
      if ((r = scan_validator(d, f.pos, f.pos + f.len, &v, &leaf)) != kNone) return r;
      for (size_t i = 0; i < entry.size() && o.vs.proposer_index < 0; i++)
        if (entry[i].len == f.len && std::memcmp(d + entry[i].pos, d + f.pos, f.len) == 0)
          o.vs.proposer_index = (int32_t)i;
      if (!entry.empty() && o.vs.proposer_index < 0) return kProposer;
    }
    // field 3, total_voting_power: canonical, and dropped as ValidatorSetFromProto drops it
  }
}

inline Reason scan_signed_header(const uint8_t *d, uint32_t lo, uint32_t hi, LightScan &o) {
  Msg m(d, lo, hi, kLightBlock);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    if (f.num == 1) {
      o.has_header = true;
      if ((r = scan_header(d, f.pos, f.pos + f.len, o.b)) != kNone) return r;
    } else {
      o.b.has_commit = true;
      if ((r = scan_commit(d, f.pos, f.pos + f.len, o.b)) != kNone) return r;
    }
  }
}

}  // namespace detail

// Scans data[lo, hi) into `o` (a fresh LightScan).  On kNone the views'
// pointers into `o` are set by finish() once `o` has its final address.
inline Reason scan_light_block(const uint8_t *data, uint32_t lo, uint32_t hi, LightScan &o) {
  using namespace detail;
  if (hi < lo) return kTruncated;
  Msg m(data, lo, hi, kLightBlock);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    if (f.num == 1) {
      o.has_signed_header = true;
      if ((r = scan_signed_header(data, f.pos, f.pos + f.len, o)) != kNone) return r;
    } else {
      o.has_vals = true;
      if ((r = scan_validator_set(data, f.pos, f.pos + f.len, o)) != kNone) return r;
    }
  }
}

// Points the views at o's own arrays; call when `o` will not move any more.
inline void finish(LightScan &o) {
  finish(o.b);
  o.sh.header = o.has_header ? &o.b.blk.header : nullptr;
  o.sh.commit = o.b.has_commit ? &o.b.commit : nullptr;
  o.vs.vals = o.vals.empty() ? nullptr : o.vals.data();
  o.vs.n_vals = (uint32_t)o.vals.size();
}

}  // namespace tmw
#pragma GCC visibility pop
