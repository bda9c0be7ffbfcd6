// tmv_merkle_wire_roots (include/tmverify.h): merkle roots over spans of one
// buffer -- a window of serialised light blocks -- whose leaves are header
// fields (tmv_merkle_span_roots' leaves) and validators (ValidatorSet.Hash
// leaves, hashed from the Validator message's own bytes).  Kept out of
// tmverify_runtime.cpp, which includes this file behind block_wire_runtime.h.
// A staged call (staged_call.h): the bytes, both tables and the tree offsets go
// up in one copy, k_span_leaves, k_valset_span_leaves and k_merkle_tree run
// (block_wire_kernels.hip, light_wire_kernels.hip), the roots come back in one
// copy.
#pragma once
#include "light_wire_hash.h"

extern "C" {

int tmv_merkle_wire_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len, const tmv_leaf_span *leaves,
                          uint32_t n_leaves, const tmv_val_span *val_leaves, uint32_t n_val_leaves,
                          const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out) {
  static const char *const who = "tmv_merkle_wire_roots";
  const std::string w(who);
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_trees == 0) return 0;
  if (!tree_off || !root_out || (n_leaves && !leaves) || (n_val_leaves && !val_leaves) || (data_len && !data)) {
    set_error(w + ": null pointer");
    return TMV_ERR_ARG;
  }
  if (n_trees > (1u << 26)) { set_error(w + ": too many trees"); return TMV_ERR_ARG; }
  const uint64_t n_all = (uint64_t)n_leaves + n_val_leaves;
  if (n_all > (1u << 26)) { set_error(w + ": too many leaves"); return TMV_ERR_ARG; }
  if (data_len > (1u << 30)) { set_error(w + ": too many data bytes"); return TMV_ERR_ARG; }
  uint32_t max_leaves = 0;
  if ((rc = offsets_rc(who, "tree_off", tree_off, n_trees, &max_leaves)) != 0) return rc;
  if (tree_off[n_trees] != n_all) {
    set_error(w + ": tree_off does not end at n_leaves + n_val_leaves");
    return TMV_ERR_ARG;
  }
  if ((rc = span_leaves_rc(w, leaves, n_leaves, data_len)) != 0) return rc;
  for (uint32_t i = 0; i < n_val_leaves; i++) {
    const tmv_val_span &v = val_leaves[i];
    // 00 || span must fit one SHA-256 block with its padding: 1 + 54 + 1 + 8
    if (v.len < 2 || v.len > 54) { set_error(w + ": validator span length outside [2, 54]"); return TMV_ERR_ARG; }
    if (v.power_at < 2 || v.power_at > v.len) { set_error(w + ": power_at outside [2, len]"); return TMV_ERR_ARG; }
    if ((uint64_t)v.pos + v.len > data_len) { set_error(w + ": validator span outside the data"); return TMV_ERR_ARG; }
  }
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  // the data first (16-byte aligned for the kernels' dword loads), 3 spare
  // bytes behind it: an aligned load of a span's last bytes stays inside
  const size_t o_data = L.in(data_len, 3), o_leaves = L.in(sizeof(tmv_leaf_span) * (size_t)n_leaves);
  const size_t o_vals = L.in(sizeof(tmv_val_span) * (size_t)n_val_leaves);
  const size_t o_toff = L.in(4ull * (n_trees + 1ull));
  const size_t o_na = L.scratch(32ull * n_all), o_nb = L.scratch(32ull * n_all);  // two node arrays
  const size_t o_out = L.out(32ull * n_trees);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_data, data, data_len);
  std::memset(c.h + o_data + data_len, 0, 3);
  c.put(o_leaves, leaves, sizeof(tmv_leaf_span) * (size_t)n_leaves);
  c.put(o_vals, val_leaves, sizeof(tmv_val_span) * (size_t)n_val_leaves);
  c.put(o_toff, tree_off, 4ull * (n_trees + 1ull));
  if ((rc = c.upload("hipMemcpyAsync(wire roots)")) != 0) return rc;
  const hipError_t e = tmv::launch_wire_roots(c.g + o_data, c.dev<const tmv_leaf_span>(o_leaves), n_leaves,
                                              c.dev<const tmv_val_span>(o_vals), n_val_leaves,
                                              c.dev<const uint32_t>(o_toff), n_trees, max_leaves,
                                              c.dev<uint32_t>(o_na), c.dev<uint32_t>(o_nb), c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("wire roots launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("wire roots readback", root_out, 32ull * n_trees);
}

}  // extern "C"
