// Column order of multi-batch launches (tmv_verify_batches_device, ed25519
// batch equation).
//
// A validator set signs every block, so entry i of every batch of a launch
// tends to carry the same public key.  The batch equation forms its groups
// from consecutive work slots; when the slots run down the columns of a tile
// of T consecutive batches (entry i of every batch of the tile, then entry
// i + 1, ...), a group holds a few long runs of one key, and k_msm_sort folds
// each run's A terms into one scalar (msm.h, "Runs of one key").
//
// For tile t = batches [tT, (t+1)T) the slot of entry i of batch j is
//   tile_base + sum_{j' in tile} min(n_j', i) + |{j' in tile : j' < j, n_j' > i}|
// -- the entries of the tile's rows above row i, then the batches before j
// that reach row i.  It needs the batches' entry counts alone and is a
// bijection onto [0, N) for ragged and empty batches too.  T = 0 or a launch
// of one batch: the identity (today's order).
//
// Compiled for the device (gather_kernels.hip) and, unchanged, for the host
// (tests/native/colorder/).
#pragma once
#include <stdint.h>
#include "curve25519.h"  // TMV_HD

namespace tmv {

constexpr uint32_t kColumnTile = 64;      // default tile height (batches)
constexpr uint32_t kColumnMaxBatches = 256;

// The batches of one launch: batch j holds the gathered entries
// [start[j], start[j + 1]).  Passed by value as a kernel argument.
struct ColumnPlan {
  uint32_t start[kColumnMaxBatches + 1];
  uint32_t K;  // batches
  uint32_t T;  // tile height; 0 = batch order
};

// Batch holding gathered entry e (start is ascending, e < start[K]): the
// search keeps start[lo] <= e < start[hi], so it ends on a non-empty batch.
TMV_HD uint32_t column_batch_of(const ColumnPlan &c, uint32_t e) {
  uint32_t lo = 0, hi = c.K;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (e >= c.start[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Work slot of entry i of batch j.
TMV_HD uint32_t column_slot(const ColumnPlan &c, uint32_t j, uint32_t i) {
  if (c.T == 0 || c.K <= 1) return c.start[j] + i;
  const uint32_t t0 = j / c.T * c.T;
  const uint32_t t1 = t0 + c.T < c.K ? t0 + c.T : c.K;
  uint32_t slot = c.start[t0];
  for (uint32_t b = t0; b < t1; b++) {
    const uint32_t nb = c.start[b + 1] - c.start[b];
    slot += nb < i ? nb : i;
    if (b < j && nb > i) slot++;
  }
  return slot;
}

}  // namespace tmv
