// merkle.Proof helpers shared by the host layer's proof translation units
// (tm_merkle_abi.cpp: part sets and Proof.Verify; tm_proof_ops_abi.cpp: value
// proof operators and tx proofs): the error-text buffer, %X, SHA-256 over
// bytes, innerHash over byte strings of any length, computeHashFromAunts and
// Proof.ValidateBasic with the reference's texts, each in one place.  Header
// only, so a build of either file without the engine needs nothing else.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/tmhost.h"
#include "merkle_plan.h"
#include "tm_light.h"

namespace tmh_proof {

using tmh::Bytes;

// The text of item i into errs + i * stride, cut to the stride.
inline void put(char *errs, size_t stride, size_t i, const std::string &s) {
  if (!errs || !stride) return;
  char *o = errs + i * stride;
  const size_t m = std::min(s.size(), stride - 1);
  std::memcpy(o, s.data(), m);
  o[m] = 0;
}

inline std::string hex_upper(const uint8_t *p, size_t n) {  // %X
  static const char d[] = "0123456789ABCDEF";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) {
    s[2 * i] = d[p[i] >> 4];
    s[2 * i + 1] = d[p[i] & 15];
  }
  return s;
}

inline void digest_out(const tmh::Digest &dg, uint8_t out[32]) {
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(dg.w[i] >> (24 - 8 * b));
}

// innerHash over byte strings of any length (computeHashFromAunts does not
// look at its aunts' sizes)
inline Bytes inner_bytes(const Bytes &l, const Bytes &r) {
  Bytes buf;
  buf.reserve(1 + l.size() + r.size());
  buf.push_back(1);
  buf.insert(buf.end(), l.begin(), l.end());
  buf.insert(buf.end(), r.begin(), r.end());
  tmh::Digest dg;
  tmh::Sha256Bytes(dg.w, nullptr, 0, buf.data(), buf.size());
  Bytes out(32);
  digest_out(dg, out.data());
  return out;
}

// computeHashFromAunts (proof.go:151-181), iteratively: the path from
// (index, total) down by split points, then the aunts folded upwards.  Empty:
// nil (or the empty leaf hash of a one-leaf tree, which bytes.Equal and %X
// do not tell from nil).
inline Bytes root_from_aunts(const tmv_proof &p) {
  if (!(p.index >= 0 && p.index < p.total)) return {};
  uint64_t t = (uint64_t)p.total, x = (uint64_t)p.index, mask = 0;
  uint32_t depth = 0;
  while (t > 1) {
    const uint64_t k = tmh::merkle_split_point(t);
    if (x < k) {
      t = k;
    } else {
      mask |= 1ull << depth;
      x -= k;
      t -= k;
    }
    depth++;
  }
  if (depth != p.n_aunts) return {};
  Bytes h(p.leaf_hash.p, p.leaf_hash.p + p.leaf_hash.len);
  for (uint32_t j = 0; j < depth; j++) {
    const Bytes a(p.aunts[j].p, p.aunts[j].p + p.aunts[j].len);
    h = ((mask >> (depth - 1 - j)) & 1) ? inner_bytes(a, h) : inner_bytes(h, a);
  }
  return h;
}

inline std::string validate_basic(const tmv_proof &p) {  // proof.go:98-117
  char buf[96];
  if (p.total < 0) return "negative Total";
  if (p.index < 0) return "negative Index";
  if (p.leaf_hash.len != 32) {
    std::snprintf(buf, sizeof buf, "expected LeafHash size to be 32, got %u", p.leaf_hash.len);
    return buf;
  }
  if (p.n_aunts > 100) {  // MaxAunts, proof.go:19
    std::snprintf(buf, sizeof buf, "expected no more than 100 aunts, got %u", p.n_aunts);
    return buf;
  }
  for (uint32_t i = 0; i < p.n_aunts; i++)
    if (p.aunts[i].len != 32) {
      std::snprintf(buf, sizeof buf, "expected Aunts#%u size to be 32, got %u", i, p.aunts[i].len);
      return buf;
    }
  return "";
}

}  // namespace tmh_proof
