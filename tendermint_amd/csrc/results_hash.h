// Device hash of ABCI tx results (results_kernels.hip): launch wrapper shared
// with the runtime (results_runtime.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmv {

// The merkle roots over abci.MarshalTxResults (abci/types/types.go:213-239) of
// n_trees lists of results: tree t holds the results [tree_off[t],
// tree_off[t+1]) of the column arrays, result i the data [data_off[i],
// data_off[i+1]).  All pointers are device pointers; data is 4-byte aligned
// and readable up to the next 4-byte boundary behind its last byte.
// first_node == nullptr: no leading leaf; tree t's leaf hashes go to node_a at
// tree_off[t] + i, and node_off is tree_off.  Else first_node holds the hashed
// leading leaf of every tree (8 words each) and node_off[t] = tree_off[t] + t:
// tree t's nodes are node_a[node_off[t] .. node_off[t+1]), the leading leaf
// first.  max_leaves: the largest tree, the leading leaf counted.  node_a /
// node_b: n_results (+ n_trees with a leading leaf) x 8 words each; out:
// n_trees x 32 B.
// One lane encodes and hashes one result whatever its length: a result of
// many KiB keeps its wave busy while the others wait, as a long message does
// in the signature kernels.
hipError_t launch_results_hashes(const uint32_t *code, const int64_t *gas_wanted, const int64_t *gas_used,
                                 const uint8_t *data, const uint32_t *data_off, uint32_t n_results,
                                 const uint32_t *tree_off, const uint32_t *node_off, uint32_t n_trees,
                                 uint32_t max_leaves, const uint32_t *first_node, uint32_t *node_a, uint32_t *node_b,
                                 uint8_t *out, hipStream_t stream);

}  // namespace tmv
