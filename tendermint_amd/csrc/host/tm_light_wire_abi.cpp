// Light blocks from their protobuf bytes (include/tmhost.h):
//   tmv_light_blocks_parse_wire      the strict scanner of light_wire.h over n
//       light blocks
//   tmv_light_blocks_validate_wire   LightBlock.ValidateBasic (types/light.go:
//       37-60) of the light blocks it handles, with Header.Hash and
//       ValidatorSet.Hash of each
// A window on the device is one tmv_merkle_wire_roots call over the caller's
// bytes -- a weak reference, as tm_block_wire_abi.cpp's: a build of this file
// without the engine (the CPU test double) loads all the same and hashes the
// views on the host with tm_light.h.  The host path re-encodes what the
// scanner decoded and the device path hashes the received bytes; the two agree
// because the scanner accepts canonical bytes only.  Only the public tmv_*
// C-ABI is used to reach the device.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "block_common.h"
#include "light_wire.h"
#include "stage_layout.h"
#include "tm_host_internal.h"
#include "tm_light.h"

extern "C" int tmv_merkle_wire_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len,
                                     const tmv_leaf_span *leaves, uint32_t n_leaves, const tmv_val_span *val_leaves,
                                     uint32_t n_val_leaves, const uint32_t *tree_off, uint32_t n_trees,
                                     uint8_t *root_out) __attribute__((weak));

namespace {

// What a tmv_light_block_views pointer points to (the C-ABI's type is never defined).
struct Views {
  std::vector<tmw::LightScan> scans;  // one per light block; emptied where it was not handled
  std::vector<int32_t> reason;
};
const Views *views_of(const tmv_light_block_views *v) { return reinterpret_cast<const Views *>(v); }
tmv_light_block_views *handle_of(Views *v) { return reinterpret_cast<tmv_light_block_views *>(v); }

using namespace tmh_block;
using tmh_internal::parallel_for;

using tmh_internal::kEngineMaxBytes;
using tmh_internal::kEngineMaxItems;

// Calls with fewer handled light blocks than this hash on the host: the light
// client's knob (tm_light_abi.cpp), read on every call here.
uint32_t device_hash_min() { return tmh_internal::env_threshold("TMV_DEVICE_HASH_MIN", 32u); }

// 0 and *out, or TMV_ERR_ARG.  *not_handled: how many light blocks were handed back.
int parse(const uint8_t *data, const uint32_t *block_off, uint32_t n, std::unique_ptr<Views> *out,
          int *not_handled) {
  if (n == 0) {
    out->reset(new Views);
    *not_handled = 0;
    return 0;
  }
  if (!block_off || tmh::check_offsets(block_off, n, nullptr) != tmh::Offsets::kOk) return TMV_ERR_ARG;
  if (block_off[n] && !data) return TMV_ERR_ARG;
  std::unique_ptr<Views> v(new Views);
  v->scans.resize(n);
  v->reason.assign(n, TMV_WIRE_REASON_NONE);
  parallel_for(n, 8, [&](size_t i) {
    tmw::LightScan &s = v->scans[i];
    const tmw::Reason r = tmw::scan_light_block(data, block_off[i], block_off[i + 1], s);
    v->reason[i] = r;
    if (r == tmw::kNone) tmw::finish(s);
    else s = tmw::LightScan();
  });
  int bad = 0;
  for (uint32_t i = 0; i < n; i++) bad += v->reason[i] != TMV_WIRE_REASON_NONE;
  *not_handled = bad;
  *out = std::move(v);
  return 0;
}

tmh::ValidatorSet vals_of(const tmv_validator_set &s) {
  tmh::ValidatorSet o;
  o.validators.resize(s.n_vals);
  for (uint32_t i = 0; i < s.n_vals; i++) {
    const tmv_validator &v = s.vals[i];
    tmh::Validator &d = o.validators[i];
    d.address = tmh::ByteView(v.address, v.address_len);
    d.pub_key.type = (tmh::KeyType)v.key_kind;
    d.pub_key.bytes = tmh::ByteView(v.pub_key, v.pub_key_len);
    d.voting_power = v.voting_power;
    d.proposer_priority = v.proposer_priority;
  }
  o.proposer = s.proposer_index;
  return o;
}

// One handled light block, converted for tm_light.h.
struct Converted {
  tmh::Header header;
  tmh::Commit commit;
  tmh::SignedHeader sh;
  tmh::ValidatorSet vs;
  tmh::Bytes header_hash, vals_hash;  // empty: nil / not computed
};

}  // namespace

extern "C" {

int tmv_light_blocks_parse_wire(const uint8_t *data, const uint32_t *block_off, uint32_t n, int32_t *reason,
                                tmv_light_block_views **out) {
  if (!out) return TMV_ERR_ARG;
  *out = nullptr;
  std::unique_ptr<Views> v;
  int bad = 0;
  const int rc = parse(data, block_off, n, &v, &bad);
  if (rc < 0) return rc;
  if (reason) std::copy(v->reason.begin(), v->reason.end(), reason);
  *out = handle_of(v.release());
  return bad;
}

const tmv_signed_header *tmv_light_block_views_header(const tmv_light_block_views *views, uint32_t i) {
  const Views *v = views_of(views);
  if (!v || i >= v->scans.size() || v->reason[i] != TMV_WIRE_REASON_NONE || !v->scans[i].has_signed_header)
    return nullptr;
  return &v->scans[i].sh;
}

const tmv_validator_set *tmv_light_block_views_vals(const tmv_light_block_views *views, uint32_t i) {
  const Views *v = views_of(views);
  if (!v || i >= v->scans.size() || v->reason[i] != TMV_WIRE_REASON_NONE || !v->scans[i].has_vals) return nullptr;
  return &v->scans[i].vs;
}

void tmv_light_block_views_free(tmv_light_block_views *v) { delete views_of(v); }

int tmv_light_blocks_validate_wire(tmv_ctx *ctx, const char *chain_id, const uint8_t *data,
                                   const uint32_t *block_off, uint32_t n, int32_t *results, int32_t *reason,
                                   char *errs, size_t err_stride, uint8_t *hash_out, uint8_t *has_hash,
                                   uint8_t *vals_hash_out, tmv_light_block_views **views_out) {
  if (views_out) *views_out = nullptr;
  if (n == 0) return 0;
  if (!results || !reason || !chain_id) return TMV_ERR_ARG;
  std::unique_ptr<Views> v;
  int bad = 0;
  int rc = parse(data, block_off, n, &v, &bad);
  if (rc < 0) return rc;
  std::vector<uint32_t> handled;
  for (uint32_t i = 0; i < n; i++)
    if (v->reason[i] == TMV_WIRE_REASON_NONE) handled.push_back(i);
  const uint32_t m = (uint32_t)handled.size();

  std::vector<Converted> cv(m);
  parallel_for(m, 16, [&](size_t k) {
    const tmw::LightScan &s = v->scans[handled[k]];
    Converted &c = cv[k];
    if (s.sh.header) {
      c.header = header_of(*s.sh.header);
      c.sh.header = &c.header;
    }
    if (s.sh.commit) {
      c.commit = commit_basic_of(*s.sh.commit);
      c.sh.commit = &c.commit;
    }
    if (s.has_vals) c.vs = vals_of(s.vs);
  });

  // what to hash: Header.Hash of every header that has one (types/block.go:
  // 448-450), ValidatorSet.Hash of every set that is there and not empty
  std::vector<uint8_t> want_header(m, 0), want_vals(m, 0);
  uint64_t span_leaves = 0, val_leaves = 0, trees = 0;
  for (uint32_t k = 0; k < m; k++) {
    const tmw::LightScan &s = v->scans[handled[k]];
    want_header[k] = s.sh.header && s.sh.header->validators_hash.len != 0;
    want_vals[k] = s.has_vals && s.vs.n_vals != 0;
    span_leaves += want_header[k] ? tmw::kHeaderLeaves : 0;
    val_leaves += want_vals[k] ? s.vs.n_vals : 0;
    trees += want_header[k] + want_vals[k];
  }
  const bool device = tmv_merkle_wire_roots && ctx && m >= device_hash_min() && trees > 0 &&
                      span_leaves + val_leaves <= kEngineMaxItems && block_off[n] <= kEngineMaxBytes;
  if (device) {
    // the header trees first, then the validator-set trees: span leaves lie in
    // front of validator leaves in the combined leaf array
    std::vector<tmv_leaf_span> table;
    std::vector<tmv_val_span> vtable;
    std::vector<uint32_t> tree_off{0};
    std::vector<tmh::Bytes *> dst;  // where tree t's root goes
    table.reserve(span_leaves);
    vtable.reserve(val_leaves);
    tree_off.reserve(trees + 1);
    dst.reserve(trees);
    for (uint32_t k = 0; k < m; k++)
      if (want_header[k]) {
        const tmw::LightScan &s = v->scans[handled[k]];
        table.insert(table.end(), s.b.hdr_leaf, s.b.hdr_leaf + tmw::kHeaderLeaves);
        tree_off.push_back((uint32_t)table.size());
        dst.push_back(&cv[k].header_hash);
      }
    for (uint32_t k = 0; k < m; k++)
      if (want_vals[k]) {
        const tmw::LightScan &s = v->scans[handled[k]];
        vtable.insert(vtable.end(), s.val_leaf.begin(), s.val_leaf.end());
        tree_off.push_back((uint32_t)(table.size() + vtable.size()));
        dst.push_back(&cv[k].vals_hash);
      }
    std::vector<uint8_t> roots(32ull * dst.size());
    rc = tmv_merkle_wire_roots(ctx, data, block_off[n], table.data(), (uint32_t)table.size(), vtable.data(),
                               (uint32_t)vtable.size(), tree_off.data(), (uint32_t)dst.size(), roots.data());
    if (rc < 0) return rc;
    for (size_t t = 0; t < dst.size(); t++) dst[t]->assign(roots.begin() + 32 * t, roots.begin() + 32 * t + 32);
  } else {
    parallel_for(m, 1, [&](size_t k) {
      if (want_header[k]) cv[k].header_hash = tmh::HeaderHashHost(cv[k].header);
      if (want_vals[k]) cv[k].vals_hash = tmh::ValidatorSetHashHost(cv[k].vs);
    });
  }

  std::vector<std::string> text(m);
  parallel_for(m, 16, [&](size_t k) {
    const tmw::LightScan &s = v->scans[handled[k]];
    const tmh::Error e = tmh::LightBlockValidateBasic(s.has_signed_header ? &cv[k].sh : nullptr,
                                                      s.has_vals ? &cv[k].vs : nullptr, chain_id, cv[k].header_hash,
                                                      cv[k].vals_hash);
    if (e) text[k] = *e;
  });

  if (hash_out) std::memset(hash_out, 0, 32ull * n);
  if (vals_hash_out) std::memset(vals_hash_out, 0, 32ull * n);
  if (has_hash) std::memset(has_hash, 0, n);
  for (uint32_t i = 0; i < n; i++) {
    results[i] = TMV_WIRE_NOT_HANDLED;
    reason[i] = v->reason[i];
    put(errs, err_stride, i, std::string());
  }
  int failed = bad;
  for (uint32_t k = 0; k < m; k++) {
    const uint32_t i = handled[k];
    results[i] = text[k].empty() ? TMV_WIRE_OK : TMV_WIRE_INVALID;
    put(errs, err_stride, i, text[k]);
    failed += results[i] != TMV_WIRE_OK;
    if (want_header[k]) {
      if (hash_out) std::memcpy(hash_out + 32ull * i, cv[k].header_hash.data(), 32);
      if (has_hash) has_hash[i] |= 1;
    }
    if (want_vals[k]) {
      if (vals_hash_out) std::memcpy(vals_hash_out + 32ull * i, cv[k].vals_hash.data(), 32);
      if (has_hash) has_hash[i] |= 2;
    }
  }
  if (views_out) *views_out = handle_of(v.release());
  return failed;
}

}  // extern "C"
