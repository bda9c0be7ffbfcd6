// A strict scanner for the protobuf bytes of a tendermint.types.Block
// (proto/tendermint/types/{block,types,evidence}.proto, version/types.proto):
// one pass, no payload copied.  Host only; needs no engine.
//
// The reference decodes a block and re-encodes pieces of it to hash them.
// Hashing the received bytes gives the same answer only if those bytes are
// what the reference's own Marshal writes for the decoded value, so the
// scanner accepts exactly the canonical gogoproto encoding and hands back
// everything else with a reason (Reason): the caller then decodes with the
// reference and takes the struct path.  Canonical means
//   * field numbers strictly ascending in a message, a repeated field's
//     entries contiguous; every known field with its declared wire type; no
//     unknown field;
//   * every varint minimal, at most 10 bytes, within 64 bits; an int32 / enum
//     the sign extension of its low 32 bits (negative: the 10-byte form); a
//     uint32 below 2^32;
//   * a zero scalar, an empty bytes and an empty string absent;
//   * the nullable = false messages present (length 0 when empty):
//     Block.header / data / evidence, Header.version / time / last_block_id,
//     BlockID.part_set_header, Commit.block_id, CommitSig.timestamp;
//     Block.last_commit present exactly when the commit is non-nil;
//   * every length inside its enclosing message;
//   * timestamps with seconds in [-62135596800, 253402300799] and nanos in
//     [0, 999999999] (outside, the reference's StdTimeUnmarshal fails).
// Not handled on purpose: a non-empty evidence list (kEvidence: checking an
// item means decoding LightBlock, ValidatorSet and Vote), and a chain_id with
// a NUL or a byte >= 0x80 (kChainID: tmv_header.chain_id is a C string, and
// UTF-8 validation differs between protobuf runtimes).  kLimit: a value the
// view structs cannot hold (a block_id_flag outside 0..255).
// The first problem in byte order is the one reported.  The bytes are a
// peer's: nothing outside [lo, hi) is read.
//
// Per handled block: a tmv_block whose hashes, addresses, signatures and
// transactions point into the caller's bytes, and the spans that
// Block.ValidateBasic hashes (tmv_leaf_span, positions from `data`):
//   sig_leaf   the payload of every `signatures` entry (Commit.Hash's leaves)
//   tx_leaf    the payload of every `txs` entry, TMV_SPAN_PREHASH
//   hdr_leaf   Header.Hash's 14 leaves (types/block.go:447-483,
//              types/encoding_helper.go): fields 1, 4 and 5 the payload; 2
//              (StringValue) and 6..14 (BytesValue) length and bytes behind
//              tag 0a; 3 (Int64Value) the varint behind tag 08; an absent
//              field the empty leaf, as cdcEncode's nil.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"

#pragma GCC visibility push(hidden)
namespace tmw {

enum Reason : int32_t {
  kNone = TMV_WIRE_REASON_NONE,
  kTruncated = TMV_WIRE_REASON_TRUNCATED,
  kWireType = TMV_WIRE_REASON_WIRE_TYPE,
  kUnknownField = TMV_WIRE_REASON_UNKNOWN_FIELD,
  kOrder = TMV_WIRE_REASON_ORDER,
  kVarint = TMV_WIRE_REASON_VARINT,
  kZeroPresent = TMV_WIRE_REASON_ZERO_PRESENT,
  kMissing = TMV_WIRE_REASON_MISSING,
  kTime = TMV_WIRE_REASON_TIME,
  kEvidence = TMV_WIRE_REASON_EVIDENCE,
  kChainID = TMV_WIRE_REASON_CHAIN_ID,
  kLimit = TMV_WIRE_REASON_LIMIT,
  // light blocks (light_wire.h)
  kKey = TMV_WIRE_REASON_KEY,
  kProposer = TMV_WIRE_REASON_PROPOSER,
  kPower = TMV_WIRE_REASON_POWER,
};

constexpr uint32_t kHeaderLeaves = 14;

struct BlockScan {
  tmv_block blk{};
  tmv_commit commit{};
  bool has_commit = false;
  std::string chain_id;  // the NUL-terminated copy blk.header.chain_id points to
  std::vector<tmv_bytes> txs;
  std::vector<tmv_commit_sig> sigs;
  std::vector<tmv_leaf_span> sig_leaf, tx_leaf;
  tmv_leaf_span hdr_leaf[kHeaderLeaves] = {};
  uint32_t max_tx = 0;  // the longest transaction
};

namespace detail {

// One message's fields, by field number (bit f of a mask: field f).
struct Spec {
  uint32_t max;       // the highest field number
  uint32_t varint;    // wire type 0; the others are length-delimited
  uint32_t message;   // embedded messages: present with length 0 is fine
  uint32_t repeated;  // entries may repeat (contiguously) and may be empty
  uint32_t required;  // nullable = false messages
};
constexpr uint32_t bit(uint32_t f) { return 1u << f; }
constexpr Spec kBlock{4, 0, bit(1) | bit(2) | bit(3) | bit(4), 0, bit(1) | bit(2) | bit(3)};
constexpr Spec kHeader{14, bit(3), bit(1) | bit(4) | bit(5), 0, bit(1) | bit(4) | bit(5)};
constexpr Spec kTwoVarints{2, bit(1) | bit(2), 0, 0, 0};  // version.Consensus, google.protobuf.Timestamp
constexpr Spec kBlockID{2, 0, bit(2), 0, bit(2)};
constexpr Spec kPartSetHeader{2, bit(1), 0, 0, 0};
constexpr Spec kData{1, 0, 0, bit(1), 0};
constexpr Spec kCommit{4, bit(1) | bit(2), bit(3) | bit(4), bit(4), bit(3)};
constexpr Spec kCommitSig{4, bit(1), bit(3), 0, bit(3)};

struct Field {
  uint32_t num = 0;
  uint64_t val = 0;   // the varint's value, or the length
  uint32_t at = 0;    // where the varint / the length begins
  uint32_t pos = 0;   // length-delimited: where the payload begins
  uint32_t len = 0;   //                   its length
};

struct Msg {
  const uint8_t *d;  // the caller's buffer; only [p, end) is read
  uint32_t p, end;
  const Spec *spec;
  uint32_t prev = 0;  // the last field number seen

  Msg(const uint8_t *d_, uint32_t lo, uint32_t hi, const Spec &s) : d(d_), p(lo), end(hi), spec(&s) {}

  Reason varint(uint64_t *out) {
    uint64_t v = 0;
    for (int i = 0; i < 10; i++) {
      if (p >= end) return kTruncated;
      const uint8_t b = d[p++];
      if (i == 9 && b > 1) return kVarint;  // beyond 64 bits, or an 11th byte follows
      v |= (uint64_t)(b & 0x7f) << (7 * i);
      if (!(b & 0x80)) {
        if (i > 0 && b == 0) return kVarint;  // padded: not minimal
        *out = v;
        return kNone;
      }
    }
    return kVarint;
  }

  // required fields in (prev, upto) are missing
  bool missing_before(uint32_t upto) const {
    for (uint32_t f = prev + 1; f < upto && f <= spec->max; f++)
      if (spec->required & bit(f)) return true;
    return false;
  }

  // The next field to *f; *more = false at the message's end.
  Reason next(Field *f, bool *more) {
    *more = false;
    if (p == end) return missing_before(spec->max + 1) ? kMissing : kNone;
    uint64_t tag;
    Reason r = varint(&tag);
    if (r != kNone) return r;
    const uint64_t num = tag >> 3;
    const uint32_t wt = (uint32_t)(tag & 7);
    if (num == 0 || num > spec->max) return kUnknownField;
    const uint32_t n = (uint32_t)num;
    if (wt != ((spec->varint & bit(n)) ? 0u : 2u)) return kWireType;
    if (n < prev || (n == prev && !(spec->repeated & bit(n)))) return kOrder;
    if (missing_before(n)) return kMissing;
    prev = n;
    f->num = n;
    f->at = p;
    if ((r = varint(&f->val)) != kNone) return r;
    if (wt == 0) {
      if (f->val == 0) return kZeroPresent;
    } else {
      if (f->val > end - p) return kTruncated;  // a length past its parent
      if (f->val == 0 && !((spec->message | spec->repeated) & bit(n))) return kZeroPresent;
      f->pos = p;
      f->len = (uint32_t)f->val;
      p += f->len;
    }
    *more = true;
    return kNone;
  }
};

inline bool is_int32(uint64_t v) { return (uint64_t)(int64_t)(int32_t)(uint32_t)v == v; }

inline Reason scan_timestamp(const uint8_t *d, uint32_t lo, uint32_t hi, int64_t *secs, int32_t *nanos) {
  Msg m(d, lo, hi, kTwoVarints);
  Field f;
  bool more;
  *secs = 0;
  *nanos = 0;
  for (;;) {
    const Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) break;
    if (f.num == 1) {
      *secs = (int64_t)f.val;
    } else {
      if (!is_int32(f.val)) return kVarint;
      *nanos = (int32_t)(uint32_t)f.val;
    }
  }
  if (*secs < -62135596800LL || *secs > 253402300799LL || *nanos < 0 || *nanos > 999999999) return kTime;
  return kNone;
}

inline Reason scan_block_id(const uint8_t *d, uint32_t lo, uint32_t hi, tmv_block_id *o) {
  *o = tmv_block_id{};
  Msg m(d, lo, hi, kBlockID);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    if (f.num == 1) {
      o->hash = d + f.pos;
      o->hash_len = f.len;
      continue;
    }
    Msg ps(d, f.pos, f.pos + f.len, kPartSetHeader);
    Field g;
    for (;;) {
      if ((r = ps.next(&g, &more)) != kNone) return r;
      if (!more) break;
      if (g.num == 1) {
        if (g.val >> 32) return kVarint;  // uint32
        o->psh_total = (uint32_t)g.val;
      } else {
        o->psh_hash = d + g.pos;
        o->psh_hash_len = g.len;
      }
    }
  }
}

inline Reason scan_commit_sig(const uint8_t *d, uint32_t lo, uint32_t hi, tmv_commit_sig *o) {
  *o = tmv_commit_sig{};
  Msg m(d, lo, hi, kCommitSig);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    switch (f.num) {
      case 1:
        if (!is_int32(f.val)) return kVarint;
        if (f.val > 255) return kLimit;
        o->block_id_flag = (uint8_t)f.val;
        break;
      case 2:
        o->validator_address = d + f.pos;
        o->validator_address_len = f.len;
        break;
      case 3:
        if ((r = scan_timestamp(d, f.pos, f.pos + f.len, &o->ts_seconds, &o->ts_nanos)) != kNone) return r;
        break;
      default:
        o->signature = d + f.pos;
        o->signature_len = f.len;
    }
  }
}

inline Reason scan_commit(const uint8_t *d, uint32_t lo, uint32_t hi, BlockScan &o) {
  Msg m(d, lo, hi, kCommit);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    switch (f.num) {
      case 1:
        o.commit.height = (int64_t)f.val;
        break;
      case 2:
        if (!is_int32(f.val)) return kVarint;
        o.commit.round = (int32_t)(uint32_t)f.val;
        break;
      case 3:
        if ((r = scan_block_id(d, f.pos, f.pos + f.len, &o.commit.block_id)) != kNone) return r;
        break;
      default: {
        tmv_commit_sig s;
        if ((r = scan_commit_sig(d, f.pos, f.pos + f.len, &s)) != kNone) return r;
        o.sigs.push_back(s);
        o.sig_leaf.push_back(tmv_leaf_span{f.pos, f.len, 0});
      }
    }
  }
}

inline Reason scan_header(const uint8_t *d, uint32_t lo, uint32_t hi, BlockScan &o) {
  tmv_header &h = o.blk.header;
  Msg m(d, lo, hi, kHeader);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    tmv_leaf_span &leaf = o.hdr_leaf[f.num - 1];
    switch (f.num) {
      case 1: {
        leaf = tmv_leaf_span{f.pos, f.len, 0};
        Msg v(d, f.pos, f.pos + f.len, kTwoVarints);
        Field g;
        for (;;) {
          if ((r = v.next(&g, &more)) != kNone) return r;
          if (!more) break;
          (g.num == 1 ? h.version_block : h.version_app) = g.val;
        }
        break;
      }
      case 2:
        for (uint32_t i = 0; i < f.len; i++)
          if (d[f.pos + i] == 0 || d[f.pos + i] >= 0x80) return kChainID;
        o.chain_id.assign(reinterpret_cast<const char *>(d + f.pos), f.len);
        leaf = tmv_leaf_span{f.at, f.pos + f.len - f.at, TMV_SPAN_TAG | 0x0a};
        break;
      case 3:
        h.height = (int64_t)f.val;
        leaf = tmv_leaf_span{f.at, m.p - f.at, TMV_SPAN_TAG | 0x08};
        break;
      case 4:
        leaf = tmv_leaf_span{f.pos, f.len, 0};
        if ((r = scan_timestamp(d, f.pos, f.pos + f.len, &h.time_seconds, &h.time_nanos)) != kNone) return r;
        break;
      case 5:
        leaf = tmv_leaf_span{f.pos, f.len, 0};
        if ((r = scan_block_id(d, f.pos, f.pos + f.len, &h.last_block_id)) != kNone) return r;
        break;
      default: {
        tmv_bytes *const dst[9] = {&h.last_commit_hash, &h.data_hash,         &h.validators_hash,
                                   &h.next_validators_hash, &h.consensus_hash, &h.app_hash,
                                   &h.last_results_hash, &h.evidence_hash,     &h.proposer_address};
        *dst[f.num - 6] = tmv_bytes{d + f.pos, f.len};
        leaf = tmv_leaf_span{f.at, f.pos + f.len - f.at, TMV_SPAN_TAG | 0x0a};
      }
    }
  }
}

}  // namespace detail

// Scans data[lo, hi) into `o` (a fresh BlockScan).  On kNone, o.blk is the
// block's view; its pointers into `o` (txs, last_commit, chain_id) are set by
// finish() once `o` has its final address.
inline Reason scan_block(const uint8_t *data, uint32_t lo, uint32_t hi, BlockScan &o) {
  using namespace detail;
  if (hi < lo) return kTruncated;
  Msg m(data, lo, hi, kBlock);
  Field f;
  bool more;
  for (;;) {
    Reason r = m.next(&f, &more);
    if (r != kNone) return r;
    if (!more) return kNone;
    switch (f.num) {
      case 1:
        if ((r = scan_header(data, f.pos, f.pos + f.len, o)) != kNone) return r;
        break;
      case 2: {
        Msg dm(data, f.pos, f.pos + f.len, kData);
        Field g;
        for (;;) {
          if ((r = dm.next(&g, &more)) != kNone) return r;
          if (!more) break;
          o.txs.push_back(tmv_bytes{data + g.pos, g.len});
          o.tx_leaf.push_back(tmv_leaf_span{g.pos, g.len, TMV_SPAN_PREHASH});
          if (g.len > o.max_tx) o.max_tx = g.len;
        }
        break;
      }
      case 3:
        if (f.len != 0) return kEvidence;
        break;
      default:
        o.has_commit = true;
        if ((r = scan_commit(data, f.pos, f.pos + f.len, o)) != kNone) return r;
    }
  }
}

// Points o.blk at o's own arrays; call when `o` will not move any more.
inline void finish(BlockScan &o) {
  o.blk.header.chain_id = o.chain_id.c_str();
  o.blk.txs = o.txs.empty() ? nullptr : o.txs.data();
  o.blk.n_txs = (uint32_t)o.txs.size();
  o.blk.evidence = nullptr;
  o.blk.n_evidence = 0;
  o.commit.sigs = o.sigs.empty() ? nullptr : o.sigs.data();
  o.commit.n_sigs = (uint32_t)o.sigs.size();
  o.blk.last_commit = o.has_commit ? &o.commit : nullptr;
}

}  // namespace tmw
#pragma GCC visibility pop
