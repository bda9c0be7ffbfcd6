// ABCI results and consensus params of the host layer (include/tmhost.h):
//   tmv_results_hash_many        merkle.HashFromByteSlices over
//       abci.MarshalTxResults (abci/types/types.go:213-239): what ApplyBlock
//       stores as State.LastResultsHash (internal/state/execution.go:262-267)
//       and validateBlock compares with the next header
//       (internal/state/validation.go:66-71)
//   tmv_consensus_params_hash    HashConsensusParams (types/params.go:385-399)
//   tmv_block_results_verify     the checks of the light client's BlockResults
//       (light/rpc/client.go:439-470)
//   tmv_consensus_params_verify  the last two checks of its ConsensusParams
//       (light/rpc/client.go:274-288)
// A large call hashes on the device through tmv_tx_results_hashes, a weak
// reference as in tm_block_abi.cpp: a build of this file without the engine
// loads all the same and computes on the host worker pool with
// results_encode.h -- the same hashes, verdicts and texts.  Only the public
// tmv_* C-ABI is used to reach the device (layering).
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "results_encode.h"
#include "tm_host_internal.h"
#include "tm_light.h"
#include "tm_proof_common.h"

extern "C" int tmv_tx_results_hashes(tmv_ctx *ctx, uint32_t flags, const uint32_t *code, const int64_t *gas_wanted,
                                     const int64_t *gas_used, const uint8_t *data, const uint32_t *data_off,
                                     const uint32_t *tree_off, uint32_t n_trees, const uint8_t *first,
                                     const uint32_t *first_off, uint8_t *root_out) __attribute__((weak));

namespace {

using tmh_internal::parallel_for;
using tmh_proof::hex_upper;
using tmh_proof::put;

constexpr uint64_t kEngineMaxItems = 1ull << 26;  // results / trees per engine call
constexpr uint64_t kEngineMaxBytes = 1ull << 30;  // data / leading-leaf bytes per engine call

// Calls with fewer results than this compute on the host.  4,096: the smallest
// swept count from which the device path, staging included, stayed ahead of
// this file's host path both without data and with 100 data bytes per result
// (without data it is ahead from 256 on; with 100 bytes the two are within
// 25 % of each other from 256 to 2,048, one way or the other; DESIGN.md
// section 21).  TMV_DEVICE_RESULTS_MIN overrides (results per call; read on
// every call: tests change it).
uint64_t device_results_min() {
  const char *e = std::getenv("TMV_DEVICE_RESULTS_MIN");
  return e ? (uint64_t)std::strtoull(e, nullptr, 10) : 4096ull;
}

// Of a call that goes to the device, a tree holding a result with more data
// bytes than this is hashed on the host: k_result_leaves hashes one result on
// one lane, so one long result would make the whole call wait for a single
// serial chain.  Swept with one long result inside a call of 100,000 results
// of 100 bytes: at 1 KiB keeping its tree on the device
// or on the host took the same time within the runs' spread, from 4 KiB on
// the host was ahead (by 13 %; at 64 KiB 4.1 times, at 1 MiB 22 times).  The
// default is the largest swept length at which the device was not behind.
// TMV_DEVICE_RESULTS_MAX_DATA overrides (bytes; read on every call).
uint64_t device_results_max_data() {
  const char *e = std::getenv("TMV_DEVICE_RESULTS_MAX_DATA");
  return e ? (uint64_t)std::strtoull(e, nullptr, 10) : 1024ull;
}

bool pointers_ok(const tmv_tx_result *rs, uint32_t n) {
  if (n && !rs) return false;
  for (uint32_t i = 0; i < n; i++)
    if (rs[i].data.len && !rs[i].data.p) return false;
  return true;
}

// One list of results with its leading leaf (null: none) and where its root goes.
struct Tree {
  const tmv_tx_result *rs;
  uint32_t n;
  const tmv_bytes *first;
  uint8_t *out;
};

// The roots of `trees`: on the device in calls within the engine's limits when
// the call is large enough, else (and for trees with a long result) on the
// host pool.  Every tree of a call has a leading leaf or none has.
int results_roots(tmv_ctx *ctx, const std::vector<Tree> &trees) {
  uint64_t total = 0;
  for (const Tree &t : trees) total += t.n;
  const bool device = tmv_tx_results_hashes && ctx && total >= device_results_min() && total > 0;
  const uint64_t max_data = device_results_max_data();
  std::vector<uint32_t> dev, host;
  for (uint32_t k = 0; k < trees.size(); k++) {
    const Tree &t = trees[k];
    bool fits = device && t.n <= kEngineMaxItems && (!t.first || t.first->len <= kEngineMaxBytes);
    uint64_t bytes = 0;
    for (uint32_t i = 0; fits && i < t.n; i++) {
      bytes += t.rs[i].data.len;
      fits = t.rs[i].data.len <= max_data && bytes <= kEngineMaxBytes;
    }
    (fits ? dev : host).push_back(k);
  }
  parallel_for(host.size(), 1, [&](size_t k) {
    const Tree &t = trees[host[k]];
    tmh::TxResultsRootHost(t.rs, t.n, t.first, t.out);
  });
  const bool lead = !trees.empty() && trees[0].first;
  for (size_t lo = 0; lo < dev.size();) {
    size_t hi = lo;
    uint64_t nr = 0, nb = 0, fb = 0;
    while (hi < dev.size()) {
      const Tree &t = trees[dev[hi]];
      uint64_t b = 0;
      for (uint32_t i = 0; i < t.n; i++) b += t.rs[i].data.len;
      const uint64_t f = lead ? t.first->len : 0;
      if (nr + t.n > kEngineMaxItems || nb + b > kEngineMaxBytes || fb + f > kEngineMaxBytes) break;
      nr += t.n;
      nb += b;
      fb += f;
      hi++;
    }
    const uint32_t m = (uint32_t)(hi - lo);  // >= 1: every tree of dev fits alone
    std::vector<uint32_t> tree_off(m + 1, 0), first_off(m + 1, 0), data_off(nr + 1, 0);
    for (uint32_t k = 0; k < m; k++) {
      const Tree &t = trees[dev[lo + k]];
      tree_off[k + 1] = tree_off[k] + t.n;
      first_off[k + 1] = first_off[k] + (lead ? t.first->len : 0);
      for (uint32_t i = 0; i < t.n; i++)
        data_off[tree_off[k] + i + 1] = data_off[tree_off[k] + i] + t.rs[i].data.len;
    }
    std::vector<uint32_t> code(std::max<uint64_t>(nr, 1));
    std::vector<int64_t> gw(std::max<uint64_t>(nr, 1)), gu(std::max<uint64_t>(nr, 1));
    std::vector<uint8_t> data(std::max<uint64_t>(nb, 1)), first(std::max<uint64_t>(fb, 1)), roots(32ull * m);
    parallel_for(m, 4, [&](size_t k) {
      const Tree &t = trees[dev[lo + k]];
      for (uint32_t i = 0; i < t.n; i++) {
        const size_t at = (size_t)tree_off[k] + i;
        code[at] = t.rs[i].code;
        gw[at] = t.rs[i].gas_wanted;
        gu[at] = t.rs[i].gas_used;
        if (t.rs[i].data.len) std::memcpy(data.data() + data_off[at], t.rs[i].data.p, t.rs[i].data.len);
      }
      if (lead && t.first->len) std::memcpy(first.data() + first_off[k], t.first->p, t.first->len);
    });
    const int rc = tmv_tx_results_hashes(ctx, lead ? TMV_RESULTS_FIRST_LEAF : 0, code.data(), gw.data(), gu.data(),
                                         data.data(), data_off.data(), tree_off.data(), m, first.data(),
                                         first_off.data(), roots.data());
    if (rc < 0) return rc;
    for (uint32_t k = 0; k < m; k++) std::memcpy(trees[dev[lo + k]].out, roots.data() + 32ull * k, 32);
    lo = hi;
  }
  return 0;
}

bool same(const uint8_t want[32], const tmv_bytes &got) { return got.len == 32 && std::memcmp(want, got.p, 32) == 0; }

const char *const kHeightText = "height must be greater than zero";  // coretypes.ErrZeroOrNegativeHeight

}  // namespace

extern "C" {

int tmv_results_hash_many(tmv_ctx *ctx, const tmv_tx_result *const *results, const uint32_t *n_results,
                          const tmv_bytes *first, uint32_t n, uint8_t *hash_out) {
  if (n == 0) return 0;
  if (!results || !n_results || !hash_out) return TMV_ERR_ARG;
  std::vector<Tree> trees(n);
  for (uint32_t i = 0; i < n; i++) {
    if (!pointers_ok(results[i], n_results[i]) || (first && first[i].len && !first[i].p)) return TMV_ERR_ARG;
    trees[i] = Tree{results[i], n_results[i], first ? first + i : nullptr, hash_out + 32ull * i};
  }
  return results_roots(ctx, trees);
}

int tmv_consensus_params_hash(int64_t block_max_bytes, int64_t block_max_gas, uint8_t out[32]) {
  if (!out) return TMV_ERR_ARG;
  tmh::ConsensusParamsHashHost(block_max_bytes, block_max_gas, out);
  return 0;
}

int tmv_block_results_verify(tmv_ctx *ctx, const tmv_block_results_in *items, uint32_t n, int32_t *results,
                             char *errs, size_t err_stride) {
  if (n == 0) return 0;
  if (!items || !results) return TMV_ERR_ARG;
  std::vector<uint8_t> roots(32ull * n);
  std::vector<Tree> trees;
  for (uint32_t i = 0; i < n; i++) {
    const tmv_block_results_in &it = items[i];
    if (!pointers_ok(it.results, it.n_results) || (it.events.len && !it.events.p) ||
        (it.last_results_hash.len && !it.last_results_hash.p))
      return TMV_ERR_ARG;
    if (it.height > 0) trees.push_back(Tree{it.results, it.n_results, &it.events, roots.data() + 32ull * i});
  }
  const int rc = results_roots(ctx, trees);
  if (rc < 0) return rc;
  int failed = 0;
  for (uint32_t i = 0; i < n; i++) {
    const tmv_block_results_in &it = items[i];
    const uint8_t *mh = roots.data() + 32ull * i;
    std::string text;
    if (it.height <= 0) text = kHeightText;
    else if (!same(mh, it.last_results_hash))
      text = "last results " + hex_upper(mh, 32) + " does not match with trusted last results " +
             hex_upper(it.last_results_hash.p, it.last_results_hash.len);
    results[i] = text.empty() ? 0 : 1;
    put(errs, err_stride, i, text);
    failed += results[i];
  }
  return failed;
}

int tmv_consensus_params_verify(tmv_ctx *, const tmv_consensus_params_in *items, uint32_t n, int32_t *results,
                                char *errs, size_t err_stride) {
  if (n == 0) return 0;
  if (!items || !results) return TMV_ERR_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (items[i].consensus_hash.len && !items[i].consensus_hash.p) return TMV_ERR_ARG;
  int failed = 0;
  for (uint32_t i = 0; i < n; i++) {
    const tmv_consensus_params_in &it = items[i];
    std::string text;
    if (it.height <= 0) {
      text = kHeightText;
    } else {
      uint8_t ch[32];
      tmh::ConsensusParamsHashHost(it.block_max_bytes, it.block_max_gas, ch);
      if (!same(ch, it.consensus_hash))
        text = "params hash " + hex_upper(ch, 32) + " does not match trusted hash " +
               hex_upper(it.consensus_hash.p, it.consensus_hash.len);
    }
    results[i] = text.empty() ? 0 : 1;
    put(errs, err_stride, i, text);
    failed += results[i];
  }
  return failed;
}

}  // extern "C"
