// Host entry points over tendermint_amd/csrc/colorder.h for
// tests/test_column_order.py and colorder_san.cpp.
#include <cstdint>
#include <vector>
#include "../../../tendermint_amd/csrc/colorder.h"

namespace {
bool make_plan(tmv::ColumnPlan &c, const uint32_t *counts, uint32_t K, uint32_t T) {
  if (K == 0 || K > tmv::kColumnMaxBatches) return false;
  uint32_t at = 0;
  for (uint32_t b = 0; b < K; b++) {
    c.start[b] = at;
    at += counts[b];
  }
  c.start[K] = at;
  c.K = K;
  c.T = T;
  return true;
}
}  // namespace

// idx_out[slot] = gathered entry, as k_column_order writes it (N words, filled
// with 0xffffffff first).  Returns the number of slots written twice or out
// of range (0 for a bijection), -1 for bad arguments.
extern "C" int64_t colordercheck_permutation(const uint32_t *counts, uint32_t K, uint32_t T, uint32_t *idx_out) {
  tmv::ColumnPlan c;
  if (!make_plan(c, counts, K, T)) return -1;
  const uint32_t N = c.start[K];
  for (uint32_t s = 0; s < N; s++) idx_out[s] = 0xffffffffu;
  int64_t bad = 0;
  for (uint32_t e = 0; e < N; e++) {
    const uint32_t j = tmv::column_batch_of(c, e);
    if (j >= K || e < c.start[j] || e >= c.start[j + 1]) { bad++; continue; }
    const uint32_t slot = tmv::column_slot(c, j, e - c.start[j]);
    if (slot >= N || idx_out[slot] != 0xffffffffu) { bad++; continue; }
    idx_out[slot] = e;
  }
  return bad;
}

// Slot of entry i of batch j.
extern "C" int64_t colordercheck_slot(const uint32_t *counts, uint32_t K, uint32_t T, uint32_t j, uint32_t i) {
  tmv::ColumnPlan c;
  if (!make_plan(c, counts, K, T) || j >= K || i >= counts[j]) return -1;
  return tmv::column_slot(c, j, i);
}
