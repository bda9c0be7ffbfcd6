// Device merkle roots over spans of one buffer (block_wire_kernels.hip):
// launch wrapper shared with the runtime (block_wire_runtime.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tmverify.h"

namespace tmv {

// Leaf i is SHA-256(00 || [tag] || data[pos, pos + len)) of leaves[i], or
// SHA-256(00 || SHA-256(span)) with TMV_SPAN_PREHASH; tree t holds the leaves
// [tree_off[t], tree_off[t+1]) and has at most max_leaves of them.  All
// pointers are device pointers; data is 4-byte aligned and readable up to the
// next 4-byte boundary behind its last byte, and every span lies inside it
// (the runtime has checked).  node_a / node_b: n_leaves x 8 words each; out:
// n_trees x 32 B.  One lane hashes one leaf whatever its length.
hipError_t launch_span_roots(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves,
                             const uint32_t *tree_off, uint32_t n_trees, uint32_t max_leaves, uint32_t *node_a,
                             uint32_t *node_b, uint8_t *out, hipStream_t stream);

// k_span_leaves alone: the leaf hashes of launch_span_roots into node (no
// launch for n_leaves == 0).
hipError_t launch_span_leaves(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves, uint32_t *node,
                              hipStream_t stream);

}  // namespace tmv
