// What the two block entry points of the host layer share
// (tm_block_abi.cpp: tmv_blocks_validate_basic over caller-built structs;
// tm_block_wire_abi.cpp: tmv_blocks_validate_wire over protobuf bytes): the
// conversion of the C structs, Block.ValidateBasic's checks in front of the
// hashes, its texts, and the host's Txs.Hash.  Not part of the public C-ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "tm_light.h"

#pragma GCC visibility push(hidden)
namespace tmh_block {

using tmh::Bytes;
using tmh::Digest;

// Calls that hash fewer commits (tmv_commit_hash_many) or validate fewer blocks
// (tmv_blocks_validate_basic, tmv_blocks_validate_wire) than this compute on
// the host: no launch on the latency path of a single block.  32 is
// tmv_header_hashes' rule; DESIGN.md section 16 has the sweep.
// TMV_DEVICE_BLOCK_MIN overrides (read on every call: tests change it).
inline uint32_t device_block_min() {
  const char *e = std::getenv("TMV_DEVICE_BLOCK_MIN");
  return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 32u;
}

inline void put(char *errs, size_t stride, size_t i, const std::string &s) {
  if (!errs || !stride) return;
  char *o = errs + i * stride;
  const size_t m = std::min(s.size(), stride - 1);
  std::memcpy(o, s.data(), m);
  o[m] = 0;
}

inline void digest_out(const Digest &dg, uint8_t out[32]) {
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(dg.w[i] >> (24 - 8 * b));
}

inline void empty_hash(uint8_t out[32]) {  // merkle emptyHash(): SHA-256("")
  Digest e;
  tmh::Sha256Bytes(e.w, nullptr, 0, nullptr, 0);
  digest_out(e, out);
}

inline tmh::ByteView view(const tmv_bytes &b) { return tmh::ByteView(b.p, b.len); }
inline Bytes copy(const uint8_t *p, size_t n) { return p && n ? Bytes(p, p + n) : Bytes(); }

inline tmh::BlockID block_id_of(const tmv_block_id &b) {
  tmh::BlockID r;
  r.hash = copy(b.hash, b.hash_len);
  r.part_set_header.total = b.psh_total;
  r.part_set_header.hash = copy(b.psh_hash, b.psh_hash_len);
  return r;
}

inline tmh::Header header_of(const tmv_header &h) {
  tmh::Header o;
  o.version_block = h.version_block;
  o.version_app = h.version_app;
  o.chain_id = h.chain_id ? h.chain_id : "";
  o.height = h.height;
  o.time = tmh::Timestamp{h.time_seconds, h.time_nanos};
  o.last_block_id = block_id_of(h.last_block_id);
  o.last_commit_hash = view(h.last_commit_hash);
  o.data_hash = view(h.data_hash);
  o.validators_hash = view(h.validators_hash);
  o.next_validators_hash = view(h.next_validators_hash);
  o.consensus_hash = view(h.consensus_hash);
  o.app_hash = view(h.app_hash);
  o.last_results_hash = view(h.last_results_hash);
  o.evidence_hash = view(h.evidence_hash);
  o.proposer_address = view(h.proposer_address);
  return o;
}

inline tmh::Commit commit_basic_of(const tmv_commit &c) {  // the parts Commit.ValidateBasic reads
  tmh::Commit o;
  o.height = c.height;
  o.round = c.round;
  o.block_id = block_id_of(c.block_id);
  o.signatures.resize(c.n_sigs);
  for (uint32_t i = 0; i < c.n_sigs; i++) {
    const tmv_commit_sig &s = c.sigs[i];
    tmh::CommitSig &d = o.signatures[i];
    d.block_id_flag = (tmh::BlockIDFlag)s.block_id_flag;
    d.validator_address = tmh::ByteView(s.validator_address, s.validator_address_len);
    d.timestamp = tmh::Timestamp{s.ts_seconds, s.ts_nanos};
    d.signature = tmh::ByteView(s.signature, s.signature_len);
  }
  return o;
}

inline tmh::Error commit_validate_basic(const tmv_commit &c) { return tmh::CommitValidateBasic(commit_basic_of(c)); }

// Block.ValidateBasic in front of the hashes (types/block.go:53-75): the text,
// empty when the block comes as far as its hashes.  *h: the converted header.
inline std::string checks_before_hashes(const tmv_block &b, tmh::Header *h) {
  *h = header_of(b.header);
  if (tmh::Error e = tmh::HeaderValidateBasic(*h)) return "invalid header: " + *e;
  if (!b.last_commit) return "nil LastCommit";
  if (tmh::Error ce = commit_validate_basic(*b.last_commit)) return "wrong LastCommit: " + *ce;
  return std::string();
}

inline bool commit_pointers_ok(const tmv_commit &c) {
  if (c.n_sigs && !c.sigs) return false;
  for (uint32_t i = 0; i < c.n_sigs; i++)
    if ((c.sigs[i].validator_address_len && !c.sigs[i].validator_address) ||
        (c.sigs[i].signature_len && !c.sigs[i].signature))
      return false;
  return true;
}

// merkle.HashFromByteSlices over items, each hashed first when prehash
// (Txs.Hash, types/tx.go:34-39), on the host.
inline void items_root_host(const tmv_bytes *items, uint32_t n, bool prehash, uint8_t out[32]) {
  if (n == 0) return empty_hash(out);
  static const uint8_t zero = 0;
  std::vector<Digest> lv(n);
  for (uint32_t i = 0; i < n; i++) {
    if (prehash) {
      Digest t;
      uint8_t tb[32];
      tmh::Sha256Bytes(t.w, nullptr, 0, items[i].p, items[i].len);
      digest_out(t, tb);
      tmh::Sha256Bytes(lv[i].w, &zero, 1, tb, 32);
    } else {
      tmh::Sha256Bytes(lv[i].w, &zero, 1, items[i].p, items[i].len);
    }
  }
  digest_out(tmh::MerkleRootHostRange(lv.data(), n), out);
}

inline std::string wrong_hash(const char *field, const uint8_t want[32], const tmv_bytes &got) {
  return std::string("wrong Header.") + field + ". Expected " + tmh::HexUpper(want, 32) + ", got " +
         tmh::HexUpper(got.p, got.len);
}

inline bool same(const uint8_t want[32], const tmv_bytes &got) {
  return got.len == 32 && std::memcmp(want, got.p, 32) == 0;
}

// The three comparisons behind the hashes (types/block.go:77-93): the text of
// the first that fails, else empty.
inline std::string compare_hashes(const tmv_header &h, const uint8_t *commit_hash, const uint8_t *data_hash,
                                  const uint8_t *evidence_hash) {
  if (!same(commit_hash, h.last_commit_hash)) return wrong_hash("LastCommitHash", commit_hash, h.last_commit_hash);
  if (!same(data_hash, h.data_hash)) return wrong_hash("DataHash", data_hash, h.data_hash);
  if (!same(evidence_hash, h.evidence_hash)) return wrong_hash("EvidenceHash", evidence_hash, h.evidence_hash);
  return std::string();
}

}  // namespace tmh_block
#pragma GCC visibility pop
