// tmv_merkle_span_roots (include/tmverify.h): merkle roots over spans of one
// buffer -- a window of serialised blocks and the table of what
// Block.ValidateBasic hashes in them -- behind the C-ABI.  Kept out of
// tmverify_runtime.cpp, which includes this file at its end.  A staged call
// (staged_call.h): the bytes, the spans and the tree offsets go up in one
// copy, k_span_leaves and k_merkle_tree run (block_wire_kernels.hip), the
// roots come back in one copy.
#pragma once
#include "block_wire_hash.h"

namespace {

// The rules of a tmv_leaf_span table over data_len bytes (tmv_merkle_span_roots,
// and the span leaves of tmv_merkle_wire_roots): 0, or TMV_ERR_ARG with "<w>: ...".
int span_leaves_rc(const std::string &w, const tmv_leaf_span *leaves, uint32_t n_leaves, uint32_t data_len) {
  for (uint32_t i = 0; i < n_leaves; i++) {
    const tmv_leaf_span &s = leaves[i];
    if (s.flags & ~(0xffu | TMV_SPAN_TAG | TMV_SPAN_PREHASH)) { set_error(w + ": unknown flag"); return TMV_ERR_ARG; }
    if ((s.flags & TMV_SPAN_TAG) && (s.flags & TMV_SPAN_PREHASH)) {
      set_error(w + ": TAG together with PREHASH");
      return TMV_ERR_ARG;
    }
    if (!(s.flags & TMV_SPAN_TAG) && (s.flags & 0xffu)) { set_error(w + ": tag byte without TAG"); return TMV_ERR_ARG; }
    if ((uint64_t)s.pos + s.len > data_len) { set_error(w + ": span outside the data"); return TMV_ERR_ARG; }
  }
  return 0;
}

}  // namespace

extern "C" {

int tmv_merkle_span_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len, const tmv_leaf_span *leaves,
                          uint32_t n_leaves, const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out) {
  static const char *const who = "tmv_merkle_span_roots";
  const std::string w(who);
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_trees == 0) return 0;
  if (!tree_off || !root_out || (n_leaves && !leaves) || (data_len && !data)) {
    set_error(w + ": null pointer");
    return TMV_ERR_ARG;
  }
  if (n_trees > (1u << 26)) { set_error(w + ": too many trees"); return TMV_ERR_ARG; }
  if (n_leaves > (1u << 26)) { set_error(w + ": too many leaves"); return TMV_ERR_ARG; }
  if (data_len > (1u << 30)) { set_error(w + ": too many data bytes"); return TMV_ERR_ARG; }
  uint32_t max_leaves = 0;
  if ((rc = offsets_rc(who, "tree_off", tree_off, n_trees, &max_leaves)) != 0) return rc;
  if (tree_off[n_trees] != n_leaves) { set_error(w + ": tree_off does not end at n_leaves"); return TMV_ERR_ARG; }
  if ((rc = span_leaves_rc(w, leaves, n_leaves, data_len)) != 0) return rc;
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  // the data first (16-byte aligned for the kernel's dword loads), 3 spare
  // bytes behind it: an aligned load of a span's last bytes stays inside
  const size_t o_data = L.in(data_len, 3), o_leaves = L.in(sizeof(tmv_leaf_span) * (size_t)n_leaves);
  const size_t o_toff = L.in(4ull * (n_trees + 1ull));
  const size_t o_na = L.scratch(32ull * n_leaves), o_nb = L.scratch(32ull * n_leaves);  // two node arrays
  const size_t o_out = L.out(32ull * n_trees);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_data, data, data_len);
  std::memset(c.h + o_data + data_len, 0, 3);
  c.put(o_leaves, leaves, sizeof(tmv_leaf_span) * (size_t)n_leaves);
  c.put(o_toff, tree_off, 4ull * (n_trees + 1ull));
  if ((rc = c.upload("hipMemcpyAsync(span roots)")) != 0) return rc;
  const hipError_t e = tmv::launch_span_roots(c.g + o_data, c.dev<const tmv_leaf_span>(o_leaves), n_leaves,
                                              c.dev<const uint32_t>(o_toff), n_trees, max_leaves,
                                              c.dev<uint32_t>(o_na), c.dev<uint32_t>(o_nb), c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("span roots launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("span roots readback", root_out, 32ull * n_trees);
}

}  // extern "C"
