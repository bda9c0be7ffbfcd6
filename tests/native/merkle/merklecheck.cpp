// C entry points over csrc/host/merkle_plan.h for tests/test_merkle_plan.py.
#include "host/merkle_plan.h"

extern "C" {

uint64_t mp_split_point(uint64_t total) { return tmh::merkle_split_point(total); }
uint32_t mp_aunt_count(uint64_t index, uint64_t total) { return tmh::merkle_aunt_count(index, total); }
int mp_aunt_offsets(const uint32_t *tree_off, uint32_t n_trees, uint32_t *out) {
  return tmh::merkle_aunt_offsets(tree_off, n_trees, out);
}
uint64_t mp_arena_base(uint32_t first_leaf, uint32_t tree) { return tmh::merkle_arena_base(first_leaf, tree); }
uint64_t mp_arena_nodes(uint32_t n_leaves, uint32_t n_trees) { return tmh::merkle_arena_nodes(n_leaves, n_trees); }
uint32_t mp_leaves_per_wave(uint32_t n_leaves) { return tmh::merkle_leaves_per_wave(n_leaves); }

}  // extern "C"
