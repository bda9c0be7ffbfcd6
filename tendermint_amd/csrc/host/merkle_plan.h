// Shape arithmetic of the merkle proof entry points (tmv_merkle_proofs,
// tmv_merkle_verify_proofs; merkle_runtime.h, merkle_proof_kernels.hip): how
// many aunts a leaf's proof holds, where each tree's upper levels sit in the
// node arena, and how many leaves a wave of the long-leaf kernel takes.  Pure
// host arithmetic with no HIP in it, unit-tested on the CPU
// (tests/test_merkle_plan.py through tests/native/merkle/).
//
// A proof's aunts (crypto/merkle/proof.go:26-31) are the siblings on the
// leaf's path to the root, so their number is the leaf's depth in the tree
// that splits at the largest power of two strictly below its size
// (crypto/merkle/tree.go:100-112); it depends on (index, total) alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tmh {

// getSplitPoint (tree.go:100-112) for total >= 2.
inline uint64_t merkle_split_point(uint64_t total) {
  return 1ull << (63 - __builtin_clzll(total - 1));
}

// Number of aunts of leaf `index` in a tree of `total` leaves
// (0 <= index < total), walking down as computeHashFromAunts does
// (proof.go:151-181).
inline uint32_t merkle_aunt_count(uint64_t index, uint64_t total) {
  uint32_t depth = 0;
  while (total > 1) {
    const uint64_t k = merkle_split_point(total);
    if (index < k) {
      total = k;
    } else {
      index -= k;
      total -= k;
    }
    depth++;
  }
  return depth;
}

// Prefix sums of the aunt counts of every leaf of n_trees trees laid out one
// after the other (tree t = leaves [tree_off[t], tree_off[t+1])): the aunts of
// leaf i are aunts[32 * out[i] .. 32 * out[i+1]).  out has tree_off[n_trees] + 1
// entries.  O(leaves): the left part of every split is a full tree, so all
// its leaves share one depth.  -1 if the offsets decrease or the count does
// not fit 32 bits.
inline int merkle_aunt_offsets(const uint32_t *tree_off, uint32_t n_trees, uint32_t *out) {
  uint64_t acc = 0;
  uint32_t leaf = 0;
  out[0] = 0;
  for (uint32_t t = 0; t < n_trees; t++) {
    if (tree_off[t + 1] < tree_off[t]) return -1;
    uint64_t n = tree_off[t + 1] - tree_off[t];
    uint32_t depth = 0;
    while (n > 1) {
      const uint64_t k = merkle_split_point(n);
      const uint32_t d = depth + 1 + (uint32_t)(63 - __builtin_clzll(k));
      for (uint64_t j = 0; j < k; j++) {
        acc += d;
        out[++leaf] = (uint32_t)acc;
      }
      n -= k;
      depth++;
    }
    if (n == 1) {
      acc += depth;
      out[++leaf] = (uint32_t)acc;
    }
    if (acc > 0xffffffffull) return -1;
  }
  return 0;
}

// Node arena of the level-keeping tree kernel: level 0 of a tree is its leaf
// hashes (the leaf kernel's output, not copied); the levels above it follow
// one another from node merkle_arena_base(tree_off[t], t).  They hold
// sum_{k>=1} ceil(n / 2^k) <= n + 32 nodes (an odd level's promoted node is
// copied up, so each of the at most 32 levels can add one), 2n + 32 per tree
// together with the leaves.
constexpr uint32_t kMerkleLevelSlack = 32;
inline uint64_t merkle_arena_base(uint32_t first_leaf, uint32_t tree) {
  return (uint64_t)first_leaf + (uint64_t)kMerkleLevelSlack * tree;
}
inline uint64_t merkle_arena_nodes(uint32_t n_leaves, uint32_t n_trees) {
  return merkle_arena_base(n_leaves, n_trees);
}

// Leaves per wave of the long-leaf kernel (8, 16, 32 or 64), set from a sweep
// of the leaf kernel over leaf counts (profiles/merkle/bench.json "lpw";
// DESIGN.md section 15 has the table).  SHA-256 is serial within a leaf and a
// wave instruction costs the same with 8 lanes active as with 64, so few
// leaves are spread thin -- but only over as many one-wave workgroups as the
// chip has CUs (256), not SIMDs: 8 per wave is fastest up to 2,048 leaves and
// 1.6x slower at 3,072, 16 per wave up to 4,096, 32 per wave up to 16,384
// (512 waves), and full waves above (24,576 leaves and more of 16 KiB).
inline uint32_t merkle_leaves_per_wave(uint32_t n_leaves) {
  if (n_leaves <= 2048) return 8;
  if (n_leaves <= 4096) return 16;
  if (n_leaves <= 16384) return 32;
  return 64;
}

}  // namespace tmh
