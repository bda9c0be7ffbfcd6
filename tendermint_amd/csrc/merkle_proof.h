// Device merkle proofs (merkle_proof_kernels.hip): launch wrappers shared
// with the runtime (merkle_runtime.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/merkle_plan.h"

namespace tmv {

constexpr uint32_t kMerkleSegBytes = 512;  // bytes of a leaf staged through LDS per round (8 SHA-256 blocks)
constexpr uint32_t kMerkleLevelSlack = tmh::kMerkleLevelSlack;

// Leaf hashes SHA-256(0x00 || leaf) (prehash: SHA-256(0x00 || SHA-256(leaf)))
// of leaves data[leaf_off[i], leaf_off[i+1]) into node (8 words per leaf).
// data: 16-byte aligned, with 16 readable bytes in front of it and readable up
// to the next 16-byte boundary behind its last byte.  lpw: leaves per wave,
// 8, 16, 32 or 64.
hipError_t launch_merkle_leaves_long(const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves, bool prehash,
                                     uint32_t lpw, uint32_t *node, hipStream_t stream);

// SHA-256(item) of items data[leaf_off[i], leaf_off[i+1]) into node (8 state
// words per item): k_merkle_leaves_long without prefix or second hash; data
// and lpw as above.
hipError_t launch_merkle_digests_long(const uint8_t *data, const uint32_t *leaf_off, uint32_t n_items, uint32_t lpw,
                                      uint32_t *node, hipStream_t stream);

// Trees over the leaf hashes leafn with every level kept in arena
// (tmh::merkle_arena_nodes(n_leaves, n_trees) x 8 words), then per leaf its
// serialised hash and, unless aunts_out is null, its aunts at aunt_off.
// root_out: n_trees x 32 B; leaf_hash_out: n_leaves x 32 B; all 16-byte aligned.
hipError_t launch_merkle_proofs(const uint32_t *tree_off, uint32_t n_trees, uint32_t n_leaves, uint32_t max_leaves,
                                const uint32_t *leafn, uint32_t *arena, const uint32_t *aunt_off, uint8_t *root_out,
                                uint8_t *leaf_hash_out, uint8_t *aunts_out, hipStream_t stream);

// Proof.Verify of n proofs; leafn: the leaves' hashes from the leaf kernel, or
// null when the leaf hash is given.  Hash arrays are 16-byte aligned.
hipError_t launch_merkle_verify_proofs(uint32_t n, const int64_t *total, const int64_t *index, const uint8_t *leaf_hash,
                                       const uint8_t *aunts, const uint32_t *aunt_off, const uint8_t *root,
                                       const uint32_t *leafn, int8_t *status_out, uint8_t *leaf_calc_out,
                                       uint8_t *root_calc_out, uint8_t *root_nil_out, hipStream_t stream);

}  // namespace tmv
