// tmv_merkle_roots / tmv_merkle_proofs / tmv_merkle_verify_proofs /
// tmv_merkle_aunt_offsets (include/tmverify.h): merkle.HashFromByteSlices
// (crypto/merkle/tree.go:11-21), ProofsFromByteSlices (proof.go:33-48) and
// Proof.Verify (proof.go:52-68) behind the C-ABI.  Kept out of
// tmverify_runtime.cpp, which includes this file at its end.  Staged calls
// (staged_call.h) with the launches of merkle_kernels.hip and
// merkle_proof_kernels.hip.
#pragma once
#include "host/merkle_plan.h"
#include "merkle_proof.h"

namespace {

// Launches whose leaves average at least this many bytes hash them with
// k_merkle_leaves_long, the others with k_merkle_leaves ($TMV_MERKLE_LONG_MIN;
// DESIGN.md "Merkle proofs" has the measurement behind the default).
uint32_t merkle_long_min() {
  static const uint32_t v = [] {
    const char *e = getenv("TMV_MERKLE_LONG_MIN");
    return e ? (uint32_t)strtoul(e, nullptr, 10) : 512u;
  }();
  return v;
}

// The checks on the leaves of n_trees trees; max_leaves out.
int merkle_check_offsets(const char *who, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                         const uint32_t *tree_off, uint32_t n_trees, uint32_t *max_leaves) {
  const std::string w(who);
  if (!leaf_off || !tree_off) { set_error(w + ": null pointer"); return TMV_ERR_ARG; }
  if (leaf_off[0] != 0 || tree_off[0] != 0 || tree_off[n_trees] != n_leaves) {
    set_error(w + ": offsets must start at 0 and tree_off must end at n_leaves");
    return TMV_ERR_ARG;
  }
  int rc = offsets_rc(who, "tree_off", tree_off, n_trees, max_leaves);
  if (rc == 0) rc = offsets_rc(who, "leaf_off", leaf_off, n_leaves);
  if (rc) return rc;
  const uint32_t bytes = leaf_off[n_leaves];
  if (bytes && !data) { set_error(w + ": null data"); return TMV_ERR_ARG; }
  if (n_leaves > (1u << 26) || bytes > (1u << 30)) { set_error(w + ": input too large"); return TMV_ERR_ARG; }
  return 0;
}

// The leaf kernel of a launch: 0 = k_merkle_leaves, else the leaves per wave
// of k_merkle_leaves_long; < 0 for flags that contradict each other.
int merkle_leaf_kernel(const char *who, uint32_t flags, uint32_t n_leaves, uint32_t bytes) {
  const uint32_t lpw = (flags >> 8) & 0xff;
  const bool force_long = (flags & TMV_MERKLE_LONG_LEAVES) || lpw, force_short = flags & TMV_MERKLE_SHORT_LEAVES;
  if ((force_long && force_short) || (force_short && (flags & TMV_MERKLE_PREHASH)) ||
      (lpw && lpw != 8 && lpw != 16 && lpw != 32 && lpw != 64)) {
    set_error(std::string(who) + ": bad flags");
    return TMV_ERR_ARG;
  }
  const bool lng = force_long || (flags & TMV_MERKLE_PREHASH) ||
                   (!force_short && n_leaves && bytes / n_leaves >= merkle_long_min());
  if (!lng) return 0;
  return lpw ? (int)lpw : (int)tmh::merkle_leaves_per_wave(n_leaves);
}

// Leaf hashes of the staged leaves (g_data has the 16 bytes of padding in
// front that k_merkle_leaves_long may read) into node.
hipError_t merkle_launch_leaves(int kernel, uint32_t flags, const uint8_t *g_data, const uint32_t *g_leaf_off,
                                uint32_t n_leaves, uint32_t *node, hipStream_t s) {
  if (kernel)
    return tmv::launch_merkle_leaves_long(g_data, g_leaf_off, n_leaves, (flags & TMV_MERKLE_PREHASH) != 0,
                                          (uint32_t)kernel, node, s);
  void *tok = tmv::ktimer::begin(tmv::ktimer::kMerkleLeaves, s);
  const hipError_t e = tmv::launch_merkle_leaves(g_data, g_leaf_off, n_leaves, node, s);
  tmv::ktimer::end(tok, s);
  return e;
}

}  // namespace

extern "C" {

int tmv_merkle_aunt_offsets(const uint32_t *tree_off, uint32_t n_trees, uint32_t *aunt_off_out) {
  if (!tree_off || !aunt_off_out) { set_error("tmv_merkle_aunt_offsets: null pointer"); return TMV_ERR_ARG; }
  const int rc = offsets_rc("tmv_merkle_aunt_offsets", "tree_off", tree_off, n_trees);
  if (rc) return rc;
  if (tree_off[n_trees] > (1u << 26)) { set_error("tmv_merkle_aunt_offsets: input too large"); return TMV_ERR_ARG; }
  if (tmh::merkle_aunt_offsets(tree_off, n_trees, aunt_off_out) != 0) {
    set_error("tmv_merkle_aunt_offsets: aunt count exceeds 32 bits");
    return TMV_ERR_ARG;
  }
  return 0;
}

int tmv_merkle_roots(tmv_ctx *ctx, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                     const uint32_t *tree_off, uint32_t n_trees, uint8_t *hash_out) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_trees == 0) return 0;
  if (!hash_out) { set_error("tmv_merkle_roots: null pointer"); return TMV_ERR_ARG; }
  uint32_t max_leaves = 0;
  if ((rc = merkle_check_offsets("tmv_merkle_roots", data, leaf_off, n_leaves, tree_off, n_trees, &max_leaves)) != 0)
    return rc;
  const uint32_t bytes = leaf_off[n_leaves];
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_leaf = L.in(4ull * (n_leaves + 1)), o_tree = L.in(4ull * (n_trees + 1)), o_data = L.in(bytes);
  const size_t o_na = L.scratch(32ull * n_leaves), o_nb = L.scratch(32ull * n_leaves);  // two node arrays
  const size_t o_out = L.out(32ull * n_trees);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_leaf, leaf_off, 4ull * (n_leaves + 1));
  c.put(o_tree, tree_off, 4ull * (n_trees + 1));
  c.put(o_data, data, bytes);
  if ((rc = c.upload("hipMemcpyAsync(merkle)")) != 0) return rc;
  const hipError_t e = tmv::launch_merkle_roots(c.g + o_data, c.dev<const uint32_t>(o_leaf), n_leaves,
                                                c.dev<const uint32_t>(o_tree), n_trees, max_leaves,
                                                c.dev<uint32_t>(o_na), c.dev<uint32_t>(o_nb), c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("merkle launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("merkle readback", hash_out, 32ull * n_trees);
}

int tmv_merkle_proofs(tmv_ctx *ctx, uint32_t flags, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                      const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out, uint8_t *leaf_hash_out,
                      const uint32_t *aunt_off, uint8_t *aunts_out) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_trees == 0) return 0;
  if (!root_out || (n_leaves && !leaf_hash_out) || (aunts_out && !aunt_off)) {
    set_error("tmv_merkle_proofs: null pointer");
    return TMV_ERR_ARG;
  }
  uint32_t max_leaves = 0;
  if ((rc = merkle_check_offsets("tmv_merkle_proofs", data, leaf_off, n_leaves, tree_off, n_trees, &max_leaves)) != 0)
    return rc;
  const uint32_t bytes = leaf_off[n_leaves];
  const int kernel = merkle_leaf_kernel("tmv_merkle_proofs", flags, n_leaves, bytes);
  if (kernel < 0) return kernel;
  uint64_t n_aunts = 0;
  if (aunts_out) {  // a leaf's aunt count follows from (index, total): the offsets must be the plan's
    std::vector<uint32_t> want((size_t)n_leaves + 1);
    if (tmh::merkle_aunt_offsets(tree_off, n_trees, want.data()) != 0 ||
        std::memcmp(want.data(), aunt_off, 4ull * (n_leaves + 1)) != 0) {
      set_error("tmv_merkle_proofs: aunt_off must come from tmv_merkle_aunt_offsets");
      return TMV_ERR_ARG;
    }
    n_aunts = aunt_off[n_leaves];
  }
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_leaf = L.in(4ull * (n_leaves + 1)), o_tree = L.in(4ull * (n_trees + 1));
  const size_t o_aunt = L.in(aunts_out ? 4ull * (n_leaves + 1) : 0), o_data = L.in_padded(bytes);
  const size_t o_leafn = L.scratch(32ull * n_leaves);  // the leaf nodes, then the arena of upper levels
  const size_t o_arena = L.scratch(32ull * tmh::merkle_arena_nodes(n_leaves, n_trees));
  const size_t o_root = L.out(32ull * n_trees), o_lh = L.out(32ull * n_leaves), o_aunts = L.out(32ull * n_aunts);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, true)) != 0) return rc;
  c.put(o_leaf, leaf_off, 4ull * (n_leaves + 1));
  c.put(o_tree, tree_off, 4ull * (n_trees + 1));
  if (aunts_out) c.put(o_aunt, aunt_off, 4ull * (n_leaves + 1));
  c.put(o_data, data, bytes);
  if ((rc = c.upload("hipMemcpyAsync(merkle proofs)")) != 0) return rc;
  uint32_t *leafn = c.dev<uint32_t>(o_leafn);
  hipError_t e = merkle_launch_leaves(kernel, flags, c.g + o_data, c.dev<const uint32_t>(o_leaf), n_leaves, leafn, c.s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_proofs(c.dev<const uint32_t>(o_tree), n_trees, n_leaves, max_leaves, leafn,
                                  c.dev<uint32_t>(o_arena), c.dev<const uint32_t>(o_aunt), c.g + o_root, c.g + o_lh,
                                  aunts_out ? c.g + o_aunts : nullptr, c.s);
  if (e != hipSuccess) { set_error("merkle proofs launch", e); return TMV_ERR_LAUNCH; }
  if ((rc = c.finish("merkle proofs readback")) != 0) return rc;
  std::memcpy(root_out, c.result(o_root), 32ull * n_trees);
  if (n_leaves) std::memcpy(leaf_hash_out, c.result(o_lh), 32ull * n_leaves);
  if (n_aunts) std::memcpy(aunts_out, c.result(o_aunts), 32ull * n_aunts);
  return 0;
}

int tmv_merkle_verify_proofs(tmv_ctx *ctx, uint32_t flags, uint32_t n, const int64_t *total, const int64_t *index,
                             const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                             const uint8_t *root, const uint8_t *data, const uint32_t *leaf_off, int8_t *status_out,
                             uint8_t *leaf_hash_calc, uint8_t *root_calc, uint8_t *root_nil) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!total || !index || !leaf_hash || !aunt_off || !root || !status_out) {
    set_error("tmv_merkle_verify_proofs: null pointer");
    return TMV_ERR_ARG;
  }
  if (n > (1u << 26)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
  if ((rc = offsets_rc("tmv_merkle_verify_proofs", "aunt_off", aunt_off, n)) != 0) return rc;
  const uint32_t n_aunts = aunt_off[n];
  if (n_aunts > (1u << 28)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
  if (n_aunts && !aunts) { set_error("tmv_merkle_verify_proofs: null aunts"); return TMV_ERR_ARG; }
  const bool given = flags & TMV_MERKLE_LEAF_HASH_GIVEN;
  uint32_t bytes = 0;
  int kernel = 0;
  if (!given) {
    if (!leaf_off) { set_error("tmv_merkle_verify_proofs: null pointer"); return TMV_ERR_ARG; }
    if ((rc = offsets_rc("tmv_merkle_verify_proofs", "leaf_off", leaf_off, n)) != 0) return rc;
    bytes = leaf_off[n];
    if (bytes && !data) { set_error("tmv_merkle_verify_proofs: null data"); return TMV_ERR_ARG; }
    if (bytes > (1u << 30)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
    kernel = merkle_leaf_kernel("tmv_merkle_verify_proofs", flags, n, bytes);
    if (kernel < 0) return kernel;
  }
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_total = L.in(8ull * n), o_index = L.in(8ull * n), o_lh = L.in(32ull * n), o_root = L.in(32ull * n);
  const size_t o_aunts = L.in(32ull * n_aunts), o_aoff = L.in(4ull * (n + 1));
  const size_t o_loff = L.in(given ? 0 : 4ull * (n + 1)), o_data = L.in_padded(bytes);
  const size_t o_leafn = L.scratch(given ? 0 : 32ull * n);  // the leaf nodes
  const size_t q_lh = L.out(32ull * n), q_root = L.out(32ull * n), q_status = L.out(n), q_nil = L.out(n);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, true)) != 0) return rc;
  c.put(o_total, total, 8ull * n);
  c.put(o_index, index, 8ull * n);
  c.put(o_lh, leaf_hash, 32ull * n);
  c.put(o_root, root, 32ull * n);
  c.put(o_aunts, aunts, 32ull * n_aunts);
  c.put(o_aoff, aunt_off, 4ull * (n + 1));
  if (!given) c.put(o_loff, leaf_off, 4ull * (n + 1));
  c.put(o_data, data, bytes);
  if ((rc = c.upload("hipMemcpyAsync(merkle verify)")) != 0) return rc;
  uint32_t *leafn = given ? nullptr : c.dev<uint32_t>(o_leafn);
  hipError_t e = hipSuccess;
  if (!given) e = merkle_launch_leaves(kernel, flags, c.g + o_data, c.dev<const uint32_t>(o_loff), n, leafn, c.s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_verify_proofs(n, c.dev<const int64_t>(o_total), c.dev<const int64_t>(o_index), c.g + o_lh,
                                         c.g + o_aunts, c.dev<const uint32_t>(o_aoff), c.g + o_root, leafn,
                                         c.dev<int8_t>(q_status), c.g + q_lh, c.g + q_root, c.g + q_nil, c.s);
  if (e != hipSuccess) { set_error("merkle verify launch", e); return TMV_ERR_LAUNCH; }
  if ((rc = c.finish("merkle verify readback")) != 0) return rc;
  std::memcpy(status_out, c.result(q_status), n);
  if (leaf_hash_calc) std::memcpy(leaf_hash_calc, c.result(q_lh), 32ull * n);
  if (root_calc) std::memcpy(root_calc, c.result(q_root), 32ull * n);
  if (root_nil) std::memcpy(root_nil, c.result(q_nil), n);
  bool all = true;
  for (uint32_t i = 0; i < n; i++) all = all && status_out[i] == 0;
  return all ? 0 : 1;
}

}  // extern "C"
