// tmv_merkle_proofs / tmv_merkle_verify_proofs / tmv_merkle_aunt_offsets
// (include/tmverify.h): merkle.ProofsFromByteSlices (crypto/merkle/proof.go:
// 33-48) and Proof.Verify (proof.go:52-68) behind the C-ABI.  Kept out of
// tmverify_runtime.cpp, which includes this file at its end: the entry points
// share its Device, staging buffers, bounded waits and error text.
// Synchronous, host buffers, device 0; staged like tmv_merkle_roots: one H2D
// copy, the launches (merkle_proof_kernels.hip), one D2H copy.
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

// The checks tmv_merkle_roots makes on its offsets; bytes and max_leaves out.
int merkle_check_offsets(const char *who, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                         const uint32_t *tree_off, uint32_t n_trees, uint32_t *max_leaves) {
  const std::string w(who);
  if (!leaf_off || !tree_off) { set_error(w + ": null pointer"); return TMV_ERR_ARG; }
  if (leaf_off[0] != 0 || tree_off[0] != 0 || tree_off[n_trees] != n_leaves) {
    set_error(w + ": offsets must start at 0 and tree_off must end at n_leaves");
    return TMV_ERR_ARG;
  }
  *max_leaves = 0;
  for (uint32_t t = 0; t < n_trees; t++) {
    if (tree_off[t + 1] < tree_off[t]) { set_error(w + ": tree_off decreasing"); return TMV_ERR_ARG; }
    *max_leaves = std::max(*max_leaves, tree_off[t + 1] - tree_off[t]);
  }
  for (uint32_t i = 0; i < n_leaves; i++)
    if (leaf_off[i + 1] < leaf_off[i]) { set_error(w + ": leaf_off decreasing"); return TMV_ERR_ARG; }
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
  if (tree_off[0] != 0) { set_error("tmv_merkle_aunt_offsets: tree_off[0] must be 0"); return TMV_ERR_ARG; }
  for (uint32_t t = 0; t < n_trees; t++)
    if (tree_off[t + 1] < tree_off[t]) { set_error("tmv_merkle_aunt_offsets: tree_off decreasing"); return TMV_ERR_ARG; }
  if (tree_off[n_trees] > (1u << 26)) { set_error("tmv_merkle_aunt_offsets: input too large"); return TMV_ERR_ARG; }
  if (tmh::merkle_aunt_offsets(tree_off, n_trees, aunt_off_out) != 0) {
    set_error("tmv_merkle_aunt_offsets: aunt count exceeds 32 bits");
    return TMV_ERR_ARG;
  }
  return 0;
}

int tmv_merkle_proofs(tmv_ctx *ctx, uint32_t flags, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                      const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out, uint8_t *leaf_hash_out,
                      const uint32_t *aunt_off, uint8_t *aunts_out) {
  if (!ctx || ctx->devs.empty()) { set_error("null context"); return TMV_ERR_ARG; }
  if (n_trees == 0) return 0;
  if (!root_out || (n_leaves && !leaf_hash_out) || (aunts_out && !aunt_off)) {
    set_error("tmv_merkle_proofs: null pointer");
    return TMV_ERR_ARG;
  }
  uint32_t max_leaves = 0;
  int rc = merkle_check_offsets("tmv_merkle_proofs", data, leaf_off, n_leaves, tree_off, n_trees, &max_leaves);
  if (rc) return rc;
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
  Device &d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.faulted) return faulted_rc(d);
  hipError_t e = hipSetDevice(d.id);
  if (e != hipSuccess) { set_error("hipSetDevice", e); return TMV_ERR_NO_DEVICE; }
  // staging: leaf_off | tree_off | aunt_off | 16 bytes of padding | data, then (device only) the leaf
  // nodes, the arena of upper levels, and the outputs roots | leaf hashes | aunts
  const size_t o_tree = align16(4ull * (n_leaves + 1)), o_aunt = o_tree + align16(4ull * (n_trees + 1));
  const size_t o_data = o_aunt + (aunts_out ? align16(4ull * (n_leaves + 1)) : 0) + 16;
  const size_t in_bytes = o_data + align16(bytes);
  const size_t o_leafn = in_bytes, o_arena = o_leafn + 32ull * n_leaves;
  const size_t o_out = o_arena + 32ull * tmh::merkle_arena_nodes(n_leaves, n_trees);
  const size_t q_leaf = 32ull * n_trees, q_aunts = q_leaf + 32ull * n_leaves, out_bytes = q_aunts + 32ull * n_aunts;
  hipStream_t s = context_stream(d);
  if (!s) { set_error("hipStreamCreate failed"); return TMV_ERR_NO_DEVICE; }
  if ((e = wait_stream(d, s)) != hipSuccess) return wait_rc(e);  // staging shared with tmv_merkle_roots
  if ((e = d.h_valset.ensure(std::max(in_bytes, out_bytes), true)) != hipSuccess) {
    set_error("hipHostMalloc", e);
    return TMV_ERR_NOMEM;
  }
  if ((e = d.d_valset.ensure(o_out + out_bytes, false)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
  uint8_t *h = static_cast<uint8_t *>(d.h_valset.ptr);
  std::memcpy(h, leaf_off, 4ull * (n_leaves + 1));
  std::memcpy(h + o_tree, tree_off, 4ull * (n_trees + 1));
  if (aunts_out) std::memcpy(h + o_aunt, aunt_off, 4ull * (n_leaves + 1));
  std::memset(h + o_data - 16, 0, 16);
  if (bytes) std::memcpy(h + o_data, data, bytes);
  uint8_t *g = static_cast<uint8_t *>(d.d_valset.ptr);
  if ((e = hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) {
    set_error("hipMemcpyAsync(merkle proofs)", e);
    return TMV_ERR_LAUNCH;
  }
  uint32_t *leafn = reinterpret_cast<uint32_t *>(g + o_leafn);
  e = merkle_launch_leaves(kernel, flags, g + o_data, reinterpret_cast<const uint32_t *>(g), n_leaves, leafn, s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_proofs(reinterpret_cast<const uint32_t *>(g + o_tree), n_trees, n_leaves, max_leaves, leafn,
                                  reinterpret_cast<uint32_t *>(g + o_arena),
                                  reinterpret_cast<const uint32_t *>(g + o_aunt), g + o_out, g + o_out + q_leaf,
                                  aunts_out ? g + o_out + q_aunts : nullptr, s);
  if (e != hipSuccess) { set_error("merkle proofs launch", e); return TMV_ERR_LAUNCH; }
  if ((e = hipMemcpyAsync(h, g + o_out, out_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = wait_stream(d, s)) != hipSuccess) {
    if (e != hipErrorNotReady) set_error("merkle proofs readback", e);
    return wait_rc(e);
  }
  std::memcpy(root_out, h, 32ull * n_trees);
  if (n_leaves) std::memcpy(leaf_hash_out, h + q_leaf, 32ull * n_leaves);
  if (n_aunts) std::memcpy(aunts_out, h + q_aunts, 32ull * n_aunts);
  return 0;
}

int tmv_merkle_verify_proofs(tmv_ctx *ctx, uint32_t flags, uint32_t n, const int64_t *total, const int64_t *index,
                             const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                             const uint8_t *root, const uint8_t *data, const uint32_t *leaf_off, int8_t *status_out,
                             uint8_t *leaf_hash_calc, uint8_t *root_calc, uint8_t *root_nil) {
  if (!ctx || ctx->devs.empty()) { set_error("null context"); return TMV_ERR_ARG; }
  if (n == 0) return 0;
  if (!total || !index || !leaf_hash || !aunt_off || !root || !status_out) {
    set_error("tmv_merkle_verify_proofs: null pointer");
    return TMV_ERR_ARG;
  }
  if (n > (1u << 26)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
  if (aunt_off[0] != 0) { set_error("tmv_merkle_verify_proofs: aunt_off[0] must be 0"); return TMV_ERR_ARG; }
  for (uint32_t i = 0; i < n; i++)
    if (aunt_off[i + 1] < aunt_off[i]) { set_error("tmv_merkle_verify_proofs: aunt_off decreasing"); return TMV_ERR_ARG; }
  const uint32_t n_aunts = aunt_off[n];
  if (n_aunts > (1u << 28)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
  if (n_aunts && !aunts) { set_error("tmv_merkle_verify_proofs: null aunts"); return TMV_ERR_ARG; }
  const bool given = flags & TMV_MERKLE_LEAF_HASH_GIVEN;
  uint32_t bytes = 0;
  int kernel = 0;
  if (!given) {
    if (!leaf_off) { set_error("tmv_merkle_verify_proofs: null pointer"); return TMV_ERR_ARG; }
    if (leaf_off[0] != 0) { set_error("tmv_merkle_verify_proofs: leaf_off[0] must be 0"); return TMV_ERR_ARG; }
    for (uint32_t i = 0; i < n; i++)
      if (leaf_off[i + 1] < leaf_off[i]) { set_error("tmv_merkle_verify_proofs: leaf_off decreasing"); return TMV_ERR_ARG; }
    bytes = leaf_off[n];
    if (bytes && !data) { set_error("tmv_merkle_verify_proofs: null data"); return TMV_ERR_ARG; }
    if (bytes > (1u << 30)) { set_error("tmv_merkle_verify_proofs: input too large"); return TMV_ERR_ARG; }
    kernel = merkle_leaf_kernel("tmv_merkle_verify_proofs", flags, n, bytes);
    if (kernel < 0) return kernel;
  }
  Device &d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.faulted) return faulted_rc(d);
  hipError_t e = hipSetDevice(d.id);
  if (e != hipSuccess) { set_error("hipSetDevice", e); return TMV_ERR_NO_DEVICE; }
  // staging: total | index | leaf hashes | roots | aunts | aunt_off | leaf_off | 16 bytes of padding | data,
  // then (device only) the leaf nodes and the outputs leaf hashes | roots | statuses | nil flags
  const size_t o_index = 8ull * n, o_lh = 2 * o_index, o_root = o_lh + 32ull * n, o_aunts = o_root + 32ull * n;
  const size_t o_aoff = o_aunts + 32ull * n_aunts, o_loff = o_aoff + align16(4ull * (n + 1));
  const size_t o_data = o_loff + (given ? 0 : align16(4ull * (n + 1))) + 16;
  const size_t in_bytes = o_data + align16(bytes);
  const size_t o_leafn = in_bytes, o_out = o_leafn + (given ? 0 : 32ull * n);
  const size_t q_root = 32ull * n, q_status = 2 * q_root, q_nil = q_status + align16(n), out_bytes = q_nil + align16(n);
  hipStream_t s = context_stream(d);
  if (!s) { set_error("hipStreamCreate failed"); return TMV_ERR_NO_DEVICE; }
  if ((e = wait_stream(d, s)) != hipSuccess) return wait_rc(e);  // staging shared with tmv_merkle_roots
  if ((e = d.h_valset.ensure(std::max(in_bytes, out_bytes), true)) != hipSuccess) {
    set_error("hipHostMalloc", e);
    return TMV_ERR_NOMEM;
  }
  if ((e = d.d_valset.ensure(o_out + out_bytes, false)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
  uint8_t *h = static_cast<uint8_t *>(d.h_valset.ptr);
  std::memcpy(h, total, 8ull * n);
  std::memcpy(h + o_index, index, 8ull * n);
  std::memcpy(h + o_lh, leaf_hash, 32ull * n);
  std::memcpy(h + o_root, root, 32ull * n);
  if (n_aunts) std::memcpy(h + o_aunts, aunts, 32ull * n_aunts);
  std::memcpy(h + o_aoff, aunt_off, 4ull * (n + 1));
  if (!given) std::memcpy(h + o_loff, leaf_off, 4ull * (n + 1));
  std::memset(h + o_data - 16, 0, 16);
  if (bytes) std::memcpy(h + o_data, data, bytes);
  uint8_t *g = static_cast<uint8_t *>(d.d_valset.ptr);
  if ((e = hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) {
    set_error("hipMemcpyAsync(merkle verify)", e);
    return TMV_ERR_LAUNCH;
  }
  uint32_t *leafn = given ? nullptr : reinterpret_cast<uint32_t *>(g + o_leafn);
  if (!given)
    e = merkle_launch_leaves(kernel, flags, g + o_data, reinterpret_cast<const uint32_t *>(g + o_loff), n, leafn, s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_verify_proofs(n, reinterpret_cast<const int64_t *>(g),
                                         reinterpret_cast<const int64_t *>(g + o_index), g + o_lh, g + o_aunts,
                                         reinterpret_cast<const uint32_t *>(g + o_aoff), g + o_root, leafn,
                                         reinterpret_cast<int8_t *>(g + o_out + q_status), g + o_out,
                                         g + o_out + q_root, g + o_out + q_nil, s);
  if (e != hipSuccess) { set_error("merkle verify launch", e); return TMV_ERR_LAUNCH; }
  if ((e = hipMemcpyAsync(h, g + o_out, out_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = wait_stream(d, s)) != hipSuccess) {
    if (e != hipErrorNotReady) set_error("merkle verify readback", e);
    return wait_rc(e);
  }
  std::memcpy(status_out, h + q_status, n);
  if (leaf_hash_calc) std::memcpy(leaf_hash_calc, h, 32ull * n);
  if (root_calc) std::memcpy(root_calc, h + q_root, 32ull * n);
  if (root_nil) std::memcpy(root_nil, h + q_nil, n);
  bool all = true;
  for (uint32_t i = 0; i < n; i++) all = all && status_out[i] == 0;
  return all ? 0 : 1;
}

}  // extern "C"
