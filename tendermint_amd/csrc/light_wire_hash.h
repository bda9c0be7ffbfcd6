// Device merkle roots over spans and validator spans of one buffer
// (light_wire_kernels.hip): launch wrapper shared with the runtime
// (light_wire_runtime.h).
#pragma once
#include "block_wire_hash.h"

namespace tmv {

// Leaves [0, n_leaves) are launch_span_roots' leaves; leaf n_leaves + v is the
// ValidatorSet.Hash leaf of vals[v]: SHA-256(00 || span) with the span's byte
// 0 replaced by 0a and, where power_at < len, its byte power_at by 10.  Tree t
// holds the leaves [tree_off[t], tree_off[t+1]) of the combined array and has
// at most max_leaves of them.  All pointers are device pointers; data as for
// launch_span_roots; every validator span lies inside it with 2 <= power_at <=
// len <= 54 (the runtime has checked).  node_a / node_b: (n_leaves + n_vals) x
// 8 words each; out: n_trees x 32 B.
hipError_t launch_wire_roots(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves,
                             const tmv_val_span *vals, uint32_t n_vals, const uint32_t *tree_off, uint32_t n_trees,
                             uint32_t max_leaves, uint32_t *node_a, uint32_t *node_b, uint8_t *out,
                             hipStream_t stream);

}  // namespace tmv
