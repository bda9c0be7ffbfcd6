// Key order of a key-merged chunk (tmverify_runtime.cpp, launch_chunk and
// stage_whole): a stable counting sort of the entries by key slot, and every
// key's segment cut at the group edges (multiples of m) into runs, which
// k_msm_items, k_msm_sort and the comb fallback read without a check.  Two
// steps, because the staging is sized by the number of distinct keys:
// key_histogram before the buffers exist, key_order_runs into them.  Host
// arithmetic only; CPU tests: tests/test_key_order.py, tests/native/keyorder/.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pool.h"

#pragma GCC visibility push(hidden)  // header-only: adds nothing to a library's exported symbols
namespace tmh {

// Chunk c counts and scatters entries [key_chunk_lo(n, c), key_chunk_lo(n, c + 1)) on a thread of its own.
constexpr uint32_t kKeySortChunks = 16;
inline uint32_t key_chunk_lo(uint32_t n, uint32_t c) { return (uint32_t)((uint64_t)n * c / kKeySortChunks); }

// hist[c * kc + k] = entries of chunk c with key slot k (kKeySortChunks * kc
// words; every slot < kc).  Returns the number of distinct slots.
inline uint32_t key_histogram(const uint32_t *slots, uint32_t n, uint32_t kc, uint32_t *hist) {
  memset(hist, 0, sizeof(uint32_t) * kKeySortChunks * kc);
  parallel_for_n(kKeySortChunks, kKeySortChunks, [&](size_t c) {
    uint32_t *hc = hist + c * kc;
    for (uint32_t j = key_chunk_lo(n, (uint32_t)c), j1 = key_chunk_lo(n, (uint32_t)c + 1); j < j1; j++) hc[slots[j]]++;
  });
  uint32_t distinct = 0;
  for (uint32_t k = 0; k < kc; k++) {
    uint32_t t = 0;
    for (uint32_t c = 0; c < kKeySortChunks; c++) t += hist[(size_t)c * kc + k];
    distinct += t != 0;
  }
  return distinct;
}

// The key-merged form is worth it while a group holds few keys: at most n / 2
// runs (every key starts a run, and so does every group edge inside one).
inline bool key_merge_worth(uint32_t distinct, uint32_t groups, uint32_t n) {
  return (uint64_t)distinct + groups <= n / 2;
}

// The run arrays as one region of 32-bit words, lo[run_cap + 1] | slot[run_cap] |
// group_run0[G + 1]: the host fills it and the device reads its copy through the same offsets.
struct KeyRunRegion {
  size_t run_cap, slot_at, group_run0_at, words;  // run_cap: a run per key, and one per group edge inside a key
  KeyRunRegion(uint32_t distinct, uint32_t G)
      : run_cap((size_t)distinct + G), slot_at(run_cap + 1), group_run0_at(2 * run_cap + 1),
        words(2 * run_cap + 1 + G + 1) {}
  size_t bytes() const { return 4 * words; }
};

// hist as key_histogram left it (used up as the sort's cursors); G groups of
// 1 << m_log2 work slots cover the n entries.  Writes
//   order[n]            the entries in key order (stable: equal keys keep their order)
//   lo[n_runs + 1]      run r covers work slots [lo[r], lo[r + 1]); lo[n_runs] == n
//   slot[n_runs]        its key slot
//   group_run0[G + 1]   group g's runs are [group_run0[g], group_run0[g + 1])
// and returns n_runs <= distinct + G.
inline uint32_t key_order_runs(uint32_t *hist, const uint32_t *slots, uint32_t n, uint32_t kc, uint32_t m_log2,
                               uint32_t G, uint32_t *order, uint32_t *lo, uint32_t *slot, uint32_t *group_run0) {
  std::vector<uint32_t> key_start(kc + 1);
  uint32_t at = 0;
  for (uint32_t k = 0; k < kc; k++) {
    key_start[k] = at;
    for (uint32_t c = 0; c < kKeySortChunks; c++) {
      const uint32_t v = hist[(size_t)c * kc + k];
      hist[(size_t)c * kc + k] = at;
      at += v;
    }
  }
  key_start[kc] = at;
  parallel_for_n(kKeySortChunks, kKeySortChunks, [&](size_t c) {
    uint32_t *cur = hist + c * kc;
    for (uint32_t j = key_chunk_lo(n, (uint32_t)c), j1 = key_chunk_lo(n, (uint32_t)c + 1); j < j1; j++)
      order[cur[slots[j]]++] = j;
  });
  // runs: key segments [key_start[k], key_start[k + 1]) cut at group edges
  const uint32_t m = 1u << m_log2;
  uint32_t n_runs = 0, g = 0;
  for (uint32_t k = 0; k < kc; k++) {
    uint32_t a0 = key_start[k];
    const uint32_t a1 = key_start[k + 1];
    while (a0 < a1) {
      while (g < G && (g << m_log2) <= a0) group_run0[g++] = n_runs;
      lo[n_runs] = a0;
      slot[n_runs] = k;
      n_runs++;
      a0 = std::min(a1, (a0 / m + 1) * m);
    }
  }
  while (g < G) group_run0[g++] = n_runs;
  lo[n_runs] = n;
  group_run0[G] = n_runs;
  return n_runs;
}

}  // namespace tmh
#pragma GCC visibility pop
