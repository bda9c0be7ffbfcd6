// Blocks from their protobuf bytes (include/tmhost.h):
//   tmv_blocks_parse_wire      the strict scanner of block_wire.h over n blocks
//   tmv_blocks_validate_wire   Block.ValidateBasic (types/block.go:53-94) of
//       the blocks it handles, with tmv_blocks_validate_basic's verdicts,
//       texts and hashes, and the part-set headers of the same bytes
// A window on the device is one tmv_merkle_span_roots call over the caller's
// bytes -- a weak reference, as tm_block_abi.cpp's: a build of this file
// without the engine (the CPU test double) loads all the same and hashes the
// views on the host with commit_encode.h and the merkle code of tm_light.h.
// The host path re-encodes what the scanner decoded and the device path hashes
// the received bytes; the two agree because the scanner accepts canonical
// bytes only.  Only the public tmv_* C-ABI is used to reach the device.
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
#include "block_wire.h"
#include "commit_encode.h"
#include "stage_layout.h"
#include "tm_host_internal.h"
#include "tm_light.h"

extern "C" int tmv_merkle_span_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len,
                                     const tmv_leaf_span *leaves, uint32_t n_leaves, const uint32_t *tree_off,
                                     uint32_t n_trees, uint8_t *root_out) __attribute__((weak));

namespace {

// What a tmv_block_views pointer points to (the C-ABI's type is never defined).
struct Views {
  std::vector<tmw::BlockScan> scans;  // one per block; emptied where the block was not handled
  std::vector<int32_t> reason;
};
const Views *views_of(const tmv_block_views *v) { return reinterpret_cast<const Views *>(v); }
tmv_block_views *handle_of(Views *v) { return reinterpret_cast<tmv_block_views *>(v); }

using namespace tmh_block;
using tmh_internal::parallel_for;

using tmh_internal::kEngineMaxBytes;
using tmh_internal::kEngineMaxItems;

// Inside a device call, a block holding a transaction of more bytes than this
// has its Data.Hash computed on the host: k_span_leaves hashes one leaf on one
// lane, so one long transaction would hold the whole call up.  The default is
// tmv_results_hash_many's for the same kernel shape.
// TMV_DEVICE_WIRE_MAX_TX overrides (read on every call).
uint32_t device_wire_max_tx() {
  return tmh_internal::env_threshold("TMV_DEVICE_WIRE_MAX_TX", 1024u);
}

// 0 and *out, or TMV_ERR_ARG.  *not_handled: how many blocks were handed back.
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
    tmw::BlockScan &s = v->scans[i];
    const tmw::Reason r = tmw::scan_block(data, block_off[i], block_off[i + 1], s);
    v->reason[i] = r;
    if (r == tmw::kNone) tmw::finish(s);
    else s = tmw::BlockScan();
  });
  int bad = 0;
  for (uint32_t i = 0; i < n; i++) bad += v->reason[i] != TMV_WIRE_REASON_NONE;
  *not_handled = bad;
  *out = std::move(v);
  return 0;
}

}  // namespace

extern "C" {

int tmv_blocks_parse_wire(const uint8_t *data, const uint32_t *block_off, uint32_t n, int32_t *reason,
                          tmv_block_views **out) {
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

const tmv_block *tmv_block_views_block(const tmv_block_views *views, uint32_t i) {
  const Views *v = views_of(views);
  if (!v || i >= v->scans.size() || v->reason[i] != TMV_WIRE_REASON_NONE) return nullptr;
  return &v->scans[i].blk;
}

void tmv_block_views_free(tmv_block_views *v) { delete views_of(v); }

int tmv_blocks_validate_wire(tmv_ctx *ctx, const uint8_t *data, const uint32_t *block_off, uint32_t n,
                             uint32_t part_size, int32_t *results, int32_t *reason, char *errs, size_t err_stride,
                             uint8_t *hash_out, uint8_t *has_hash, uint32_t *psh_total_out, uint8_t *psh_hash_out,
                             tmv_block_views **views_out) {
  if (views_out) *views_out = nullptr;
  if (n == 0) return 0;
  if (!results || !reason || (part_size && (!psh_total_out || !psh_hash_out))) return TMV_ERR_ARG;
  std::unique_ptr<Views> v;
  int bad = 0;
  int rc = parse(data, block_off, n, &v, &bad);
  if (rc < 0) return rc;
  std::vector<uint32_t> handled;
  for (uint32_t i = 0; i < n; i++)
    if (v->reason[i] == TMV_WIRE_REASON_NONE) handled.push_back(i);
  const uint32_t m = (uint32_t)handled.size();

  // Header.ValidateBasic, nil LastCommit, Commit.ValidateBasic
  std::vector<tmh::Header> hs(m);
  std::vector<std::string> text(m);
  parallel_for(m, 16, [&](size_t k) { text[k] = checks_before_hashes(v->scans[handled[k]].blk, &hs[k]); });

  // what to hash: Commit.Hash and Data.Hash of the blocks that came this far,
  // Header.Hash of every header that has one (types/block.go:448-450)
  std::vector<uint8_t> commit_hash(32ull * std::max<uint32_t>(m, 1)), data_hash(commit_hash.size()),
      header_hash(commit_hash.size()), evidence_hash(32);
  empty_hash(evidence_hash.data());  // a handled block has no evidence
  std::vector<uint8_t> want_header(m, 0), on_device(m, 0), tx_on_device(m, 0);
  uint64_t leaves = 0, trees = 0;
  const uint32_t max_tx = device_wire_max_tx();
  for (uint32_t k = 0; k < m; k++) {
    const tmw::BlockScan &s = v->scans[handled[k]];
    want_header[k] = hash_out && s.blk.header.validators_hash.len != 0;
    if (text[k].empty()) {
      tx_on_device[k] = s.max_tx <= max_tx;
      leaves += s.sig_leaf.size() + (tx_on_device[k] ? s.tx_leaf.size() : 0);
      trees += 1 + tx_on_device[k];
    }
    if (want_header[k]) {
      leaves += tmw::kHeaderLeaves;
      trees++;
    }
  }
  const bool device = tmv_merkle_span_roots && ctx && m >= device_block_min() && trees > 0 &&
                      leaves <= kEngineMaxItems && trees <= kEngineMaxItems && block_off[n] <= kEngineMaxBytes;
  if (device) {
    // leaves grouped by kind across the window, so that a wave holds leaves of
    // one shape: the commit signatures, the transactions, the header fields
    std::vector<tmv_leaf_span> table;
    std::vector<uint32_t> tree_off{0};
    std::vector<uint8_t *> dst;  // where tree t's root goes
    table.reserve(leaves);
    tree_off.reserve(trees + 1);
    dst.reserve(trees);
    auto add = [&](const tmv_leaf_span *p, size_t cnt, uint8_t *to) {
      table.insert(table.end(), p, p + cnt);
      tree_off.push_back((uint32_t)table.size());
      dst.push_back(to);
    };
    for (uint32_t k = 0; k < m; k++)
      if (text[k].empty()) {
        const tmw::BlockScan &s = v->scans[handled[k]];
        add(s.sig_leaf.data(), s.sig_leaf.size(), commit_hash.data() + 32ull * k);
        on_device[k] = 1;
      }
    for (uint32_t k = 0; k < m; k++)
      if (text[k].empty() && tx_on_device[k]) {
        const tmw::BlockScan &s = v->scans[handled[k]];
        add(s.tx_leaf.data(), s.tx_leaf.size(), data_hash.data() + 32ull * k);
      }
    for (uint32_t k = 0; k < m; k++)
      if (want_header[k]) add(v->scans[handled[k]].hdr_leaf, tmw::kHeaderLeaves, header_hash.data() + 32ull * k);
    std::vector<uint8_t> roots(32ull * dst.size());
    rc = tmv_merkle_span_roots(ctx, data, block_off[n], table.data(), (uint32_t)table.size(), tree_off.data(),
                               (uint32_t)dst.size(), roots.data());
    if (rc < 0) return rc;
    for (size_t t = 0; t < dst.size(); t++) std::memcpy(dst[t], roots.data() + 32ull * t, 32);
  }
  // on the host: everything of a host call, and the long transactions of a device call
  parallel_for(m, 1, [&](size_t k) {
    const tmw::BlockScan &s = v->scans[handled[k]];
    if (text[k].empty()) {
      if (!on_device[k]) tmh::CommitHashHost(s.commit, commit_hash.data() + 32ull * k);
      if (!device || !tx_on_device[k]) items_root_host(s.blk.txs, s.blk.n_txs, true, data_hash.data() + 32ull * k);
    }
    if (want_header[k] && !device) {
      const Bytes h = tmh::HeaderHashHost(hs[k]);
      std::memcpy(header_hash.data() + 32ull * k, h.data(), 32);
    }
  });

  if (hash_out) std::memset(hash_out, 0, 32ull * n);
  if (has_hash) std::memset(has_hash, 0, n);
  for (uint32_t i = 0; i < n; i++) {
    results[i] = TMV_WIRE_NOT_HANDLED;
    reason[i] = v->reason[i];
    put(errs, err_stride, i, std::string());
  }
  int failed = bad;
  for (uint32_t k = 0; k < m; k++) {
    const uint32_t i = handled[k];
    if (text[k].empty())
      text[k] = compare_hashes(v->scans[i].blk.header, commit_hash.data() + 32ull * k, data_hash.data() + 32ull * k,
                               evidence_hash.data());
    results[i] = text[k].empty() ? TMV_WIRE_OK : TMV_WIRE_INVALID;
    put(errs, err_stride, i, text[k]);
    failed += results[i] != TMV_WIRE_OK;
    if (want_header[k]) {
      std::memcpy(hash_out + 32ull * i, header_hash.data() + 32ull * k, 32);
      if (has_hash) has_hash[i] = 1;
    }
  }

  if (part_size) {
    std::vector<tmv_bytes> raws(n);
    for (uint32_t i = 0; i < n; i++) raws[i] = tmv_bytes{data + block_off[i], block_off[i + 1] - block_off[i]};
    rc = tmv_part_set_headers(ctx, raws.data(), n, part_size, psh_total_out, psh_hash_out);
    if (rc < 0) return rc;
  }
  if (views_out) *views_out = handle_of(v.release());
  return failed;
}

}  // extern "C"
