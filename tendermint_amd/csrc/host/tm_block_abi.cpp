// Blocks of the host layer (include/tmhost.h):
//   tmv_commit_hash_many        Commit.Hash (types/block.go:900-918)
//   tmv_blocks_validate_basic   Block.ValidateBasic (types/block.go:53-94), the
//       first step of ValidateBlock (internal/state/validation.go:16) that
//       blocksync runs on every block it applies
//       (internal/blocksync/reactor.go:563-586): it ties the header that the
//       commit signs to the block's last commit, transactions and evidence.
// A window of blocks hashes on the device: all last commits in one
// tmv_commit_hashes launch, all Data.Hash trees in one tmv_merkle_proofs call,
// the evidence trees in one tmv_merkle_roots call, the headers through
// tmv_header_hashes -- weak references, as tm_merkle_abi.cpp's: a build of
// this file without the engine (the CPU test double) loads all the same and
// computes on the host with commit_encode.h and the merkle code of tm_light.h,
// the same hashes, verdicts and texts.  Only the public tmv_* C-ABI is used to
// reach the device (layering).
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
#include "commit_encode.h"
#include "tm_host_internal.h"
#include "tm_light.h"

extern "C" int tmv_commit_hashes(tmv_ctx *ctx, const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                                 const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len,
                                 const uint8_t *sig, const uint32_t *commit_off, uint32_t n_commits,
                                 uint8_t *hash_out) __attribute__((weak));
extern "C" int tmv_merkle_proofs(tmv_ctx *ctx, uint32_t flags, const uint8_t *data, const uint32_t *leaf_off,
                                 uint32_t n_leaves, const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out,
                                 uint8_t *leaf_hash_out, const uint32_t *aunt_off, uint8_t *aunts_out)
    __attribute__((weak));
extern "C" int tmv_merkle_roots(tmv_ctx *ctx, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                                const uint32_t *tree_off, uint32_t n_trees, uint8_t *hash_out) __attribute__((weak));
extern "C" int tmv_header_hashes(tmv_ctx *ctx, const tmv_header *headers, uint32_t n, uint8_t *hash_out,
                                 uint8_t *has_hash) __attribute__((weak));

namespace {

using namespace tmh_block;
using tmh_internal::parallel_for;

constexpr uint64_t kEngineMaxItems = 1ull << 26;  // signatures / leaves per engine call
constexpr uint64_t kEngineMaxBytes = 1ull << 30;  // leaf bytes per engine call

bool engine_accepts(const tmv_commit &c) {  // tmv_commit_hashes' fixed columns
  for (uint32_t i = 0; i < c.n_sigs; i++) {
    const tmv_commit_sig &s = c.sigs[i];
    if (s.block_id_flag > 127 || (s.validator_address_len != 0 && s.validator_address_len != 20) ||
        s.signature_len > 64)
      return false;
  }
  return c.n_sigs <= kEngineMaxItems;
}

// Commit.Hash of each (non-nil) commit to out + 32*i.  With `device`, the
// commits the engine accepts go to it, in calls of at most 2^26 signatures.
int commit_hashes(tmv_ctx *ctx, const std::vector<const tmv_commit *> &cs, uint8_t *out, bool device) {
  std::vector<uint32_t> dev, host;
  for (uint32_t i = 0; i < cs.size(); i++) (device && engine_accepts(*cs[i]) ? dev : host).push_back(i);
  parallel_for(host.size(), 1, [&](size_t k) { tmh::CommitHashHost(*cs[host[k]], out + 32ull * host[k]); });
  for (size_t lo = 0; lo < dev.size();) {
    size_t hi = lo;
    uint64_t total = 0;
    while (hi < dev.size() && total + cs[dev[hi]]->n_sigs <= kEngineMaxItems) total += cs[dev[hi++]]->n_sigs;
    const uint32_t m = (uint32_t)(hi - lo);
    std::vector<uint32_t> off(m + 1, 0);
    for (uint32_t k = 0; k < m; k++) off[k + 1] = off[k] + cs[dev[lo + k]]->n_sigs;
    const size_t cap = std::max<size_t>(total, 1);
    std::vector<uint8_t> flag(cap), alen(cap), slen(cap), addr(20 * cap), sig(64 * cap);
    std::vector<int64_t> sec(cap);
    std::vector<int32_t> nan(cap);
    parallel_for(m, 16, [&](size_t k) {
      const tmv_commit &c = *cs[dev[lo + k]];
      for (uint32_t j = 0; j < c.n_sigs; j++) {
        const tmv_commit_sig &s = c.sigs[j];
        const size_t i = (size_t)off[k] + j;
        flag[i] = s.block_id_flag;
        alen[i] = (uint8_t)s.validator_address_len;
        slen[i] = (uint8_t)s.signature_len;
        sec[i] = s.ts_seconds;
        nan[i] = s.ts_nanos;
        if (s.validator_address_len) std::memcpy(addr.data() + 20 * i, s.validator_address, 20);
        if (s.signature_len) std::memcpy(sig.data() + 64 * i, s.signature, s.signature_len);
      }
    });
    std::vector<uint8_t> roots(32ull * m);
    const int rc = tmv_commit_hashes(ctx, flag.data(), alen.data(), addr.data(), sec.data(), nan.data(), slen.data(),
                                     sig.data(), off.data(), m, roots.data());
    if (rc < 0) return rc;
    for (uint32_t k = 0; k < m; k++) std::memcpy(out + 32ull * dev[lo + k], roots.data() + 32ull * k, 32);
    lo = hi;
  }
  return 0;
}

// One list of byte strings per block (transactions or evidence).
struct Lists {
  const tmv_block *blocks;
  bool txs;
  const tmv_bytes *items(uint32_t b) const { return txs ? blocks[b].txs : blocks[b].evidence; }
  uint32_t count(uint32_t b) const { return txs ? blocks[b].n_txs : blocks[b].n_evidence; }
};

// The merkle root of each listed block's items to out + 32*block.  With
// `device`, one engine call for all of them when it fits the engine's limits.
int list_roots(tmv_ctx *ctx, const Lists &ls, const std::vector<uint32_t> &who, uint8_t *out, bool device) {
  uint64_t leaves = 0, bytes = 0;
  for (uint32_t b : who) {
    leaves += ls.count(b);
    for (uint32_t i = 0; i < ls.count(b); i++) bytes += ls.items(b)[i].len;
  }
  if (leaves == 0) {  // every tree is empty: the constant, no launch
    for (uint32_t b : who) empty_hash(out + 32ull * b);
    return 0;
  }
  if (!device || leaves > kEngineMaxItems || bytes > kEngineMaxBytes) {
    parallel_for(who.size(), 1, [&](size_t k) {
      items_root_host(ls.items(who[k]), ls.count(who[k]), ls.txs, out + 32ull * who[k]);
    });
    return 0;
  }
  const uint32_t m = (uint32_t)who.size();
  std::vector<uint32_t> tree_off(m + 1, 0), leaf_off(leaves + 1, 0);
  for (uint32_t k = 0; k < m; k++) {
    const uint32_t b = who[k];
    tree_off[k + 1] = tree_off[k] + ls.count(b);
    for (uint32_t i = 0; i < ls.count(b); i++)
      leaf_off[tree_off[k] + i + 1] = leaf_off[tree_off[k] + i] + ls.items(b)[i].len;
  }
  std::vector<uint8_t> data(std::max<uint64_t>(bytes, 1)), roots(32ull * m);
  parallel_for(m, 4, [&](size_t k) {
    const uint32_t b = who[k];
    for (uint32_t i = 0; i < ls.count(b); i++)
      if (ls.items(b)[i].len) std::memcpy(data.data() + leaf_off[tree_off[k] + i], ls.items(b)[i].p, ls.items(b)[i].len);
  });
  int rc;
  if (ls.txs) {  // roots only: no aunts
    std::vector<uint8_t> leaf_hashes(32ull * leaves);
    rc = tmv_merkle_proofs(ctx, TMV_MERKLE_PREHASH, bytes ? data.data() : nullptr, leaf_off.data(), (uint32_t)leaves,
                           tree_off.data(), m, roots.data(), leaf_hashes.data(), nullptr, nullptr);
  } else {
    rc = tmv_merkle_roots(ctx, bytes ? data.data() : nullptr, leaf_off.data(), (uint32_t)leaves, tree_off.data(), m,
                          roots.data());
  }
  if (rc < 0) return rc;
  for (uint32_t k = 0; k < m; k++) std::memcpy(out + 32ull * who[k], roots.data() + 32ull * k, 32);
  return 0;
}

}  // namespace

extern "C" {

int tmv_commit_hash_many(tmv_ctx *ctx, const tmv_commit *const *commits, uint32_t n, uint8_t *hash_out,
                         uint8_t *has_hash) {
  if (n == 0) return 0;
  if (!commits || !hash_out) return TMV_ERR_ARG;
  std::vector<const tmv_commit *> cs;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < n; i++) {
    if (has_hash) has_hash[i] = commits[i] ? 1 : 0;
    if (!commits[i]) continue;
    if (!commit_pointers_ok(*commits[i])) return TMV_ERR_ARG;
    cs.push_back(commits[i]);
    who.push_back(i);
  }
  uint32_t accepted = 0;
  for (const tmv_commit *c : cs) accepted += engine_accepts(*c);
  const bool device = tmv_commit_hashes && ctx && accepted >= device_block_min();
  std::vector<uint8_t> out(32ull * std::max<size_t>(cs.size(), 1));
  const int rc = commit_hashes(ctx, cs, out.data(), device);
  if (rc < 0) return rc;
  std::memset(hash_out, 0, 32ull * n);
  for (size_t k = 0; k < who.size(); k++) std::memcpy(hash_out + 32ull * who[k], out.data() + 32ull * k, 32);
  return 0;
}

int tmv_blocks_validate_basic(tmv_ctx *ctx, const tmv_block *blocks, uint32_t n, int32_t *results, char *errs,
                              size_t err_stride, uint8_t *hash_out, uint8_t *has_hash) {
  if (n == 0) return 0;
  if (!blocks || !results) return TMV_ERR_ARG;
  for (uint32_t b = 0; b < n; b++) {
    const tmv_block &k = blocks[b];
    if ((k.n_txs && !k.txs) || (k.n_evidence && !k.evidence)) return TMV_ERR_ARG;
    for (uint32_t i = 0; i < k.n_txs; i++)
      if (k.txs[i].len && !k.txs[i].p) return TMV_ERR_ARG;
    for (uint32_t i = 0; i < k.n_evidence; i++)
      if (k.evidence[i].len && !k.evidence[i].p) return TMV_ERR_ARG;
    if (k.last_commit && !commit_pointers_ok(*k.last_commit)) return TMV_ERR_ARG;
  }
  const bool device = ctx && n >= device_block_min();

  // Header.ValidateBasic, nil LastCommit, Commit.ValidateBasic
  std::vector<tmh::Header> hs(n);
  std::vector<std::string> text(n);
  parallel_for(n, 16, [&](size_t b) { text[b] = checks_before_hashes(blocks[b], &hs[b]); });

  // Header.Hash of every header as given
  if (hash_out) {
    std::vector<uint8_t> has(n, 0);
    if (device && tmv_header_hashes) {
      std::vector<tmv_header> flat(n);
      for (uint32_t b = 0; b < n; b++) flat[b] = blocks[b].header;
      const int rc = tmv_header_hashes(ctx, flat.data(), n, hash_out, has.data());
      if (rc < 0) return rc;
    } else {
      std::memset(hash_out, 0, 32ull * n);
      parallel_for(n, 16, [&](size_t b) {
        const Bytes h = tmh::HeaderHashHost(hs[b]);
        has[b] = h.empty() ? 0 : 1;
        if (!h.empty()) std::memcpy(hash_out + 32ull * b, h.data(), 32);
      });
    }
    if (has_hash) std::memcpy(has_hash, has.data(), n);
  }

  // the three hashes of the blocks that came this far
  std::vector<uint32_t> live;
  std::vector<const tmv_commit *> cs;
  for (uint32_t b = 0; b < n; b++)
    if (text[b].empty()) {
      live.push_back(b);
      cs.push_back(blocks[b].last_commit);
    }
  std::vector<uint8_t> commit_hash(32ull * std::max<size_t>(live.size(), 1)), data_hash(32ull * n),
      evidence_hash(32ull * n);
  int rc = commit_hashes(ctx, cs, commit_hash.data(), device && tmv_commit_hashes);
  if (rc < 0) return rc;
  rc = list_roots(ctx, Lists{blocks, true}, live, data_hash.data(), device && tmv_merkle_proofs);
  if (rc < 0) return rc;
  rc = list_roots(ctx, Lists{blocks, false}, live, evidence_hash.data(), device && tmv_merkle_roots);
  if (rc < 0) return rc;
  for (size_t k = 0; k < live.size(); k++) {
    const uint32_t b = live[k];
    const tmv_header &h = blocks[b].header;
    const uint8_t *ch = commit_hash.data() + 32ull * k, *dh = data_hash.data() + 32ull * b,
                  *eh = evidence_hash.data() + 32ull * b;
    text[b] = compare_hashes(h, ch, dh, eh);
  }

  int failed = 0;
  for (uint32_t b = 0; b < n; b++) {
    results[b] = text[b].empty() ? 0 : 1;
    put(errs, err_stride, b, text[b]);
    failed += results[b];
  }
  return failed;
}

}  // extern "C"
