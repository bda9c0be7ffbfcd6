// tmv_tx_results_hashes (include/tmverify.h): the merkle roots over
// abci.MarshalTxResults (abci/types/types.go:213-239) of many blocks' results
// behind the C-ABI.  Kept out of tmverify_runtime.cpp, which includes this
// file at its end, after merkle_runtime.h, whose choice of leaf kernel hashes
// the leading leaves.  A staged call (staged_call.h) with the launches of
// results_kernels.hip.
#pragma once
#include "results_hash.h"

extern "C" {

int tmv_tx_results_hashes(tmv_ctx *ctx, uint32_t flags, const uint32_t *code, const int64_t *gas_wanted,
                          const int64_t *gas_used, const uint8_t *data, const uint32_t *data_off,
                          const uint32_t *tree_off, uint32_t n_trees, const uint8_t *first, const uint32_t *first_off,
                          uint8_t *root_out) {
  static const char *const who = "tmv_tx_results_hashes";
  const std::string w(who);
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (flags & ~TMV_RESULTS_FIRST_LEAF) { set_error(w + ": unknown flag"); return TMV_ERR_ARG; }
  if (n_trees == 0) return 0;
  const bool lead = flags & TMV_RESULTS_FIRST_LEAF;
  if (!tree_off || !root_out || (lead && !first_off)) { set_error(w + ": null pointer"); return TMV_ERR_ARG; }
  if (n_trees > (1u << 26)) { set_error(w + ": too many trees"); return TMV_ERR_ARG; }
  uint32_t max_leaves = 0, first_bytes = 0;
  if ((rc = offsets_rc(who, "tree_off", tree_off, n_trees, &max_leaves)) != 0) return rc;
  const uint32_t n = tree_off[n_trees];
  if (n > (1u << 26)) { set_error(w + ": too many results"); return TMV_ERR_ARG; }
  if (n && (!code || !gas_wanted || !gas_used || !data_off)) { set_error(w + ": null pointer"); return TMV_ERR_ARG; }
  uint32_t bytes = 0;
  if (n) {
    if ((rc = offsets_rc(who, "data_off", data_off, n)) != 0) return rc;
    bytes = data_off[n];
  }
  if (lead) {
    if ((rc = offsets_rc(who, "first_off", first_off, n_trees)) != 0) return rc;
    first_bytes = first_off[n_trees];
  }
  if ((bytes && !data) || (first_bytes && !first)) { set_error(w + ": null data"); return TMV_ERR_ARG; }
  if (bytes > (1u << 30) || first_bytes > (1u << 30)) { set_error(w + ": too many data bytes"); return TMV_ERR_ARG; }
  const int kernel = lead ? merkle_leaf_kernel(who, 0, n_trees, first_bytes) : 0;  // of the leading leaves
  if (kernel < 0) return kernel;
  if ((rc = c.open()) != 0) return rc;
  const uint32_t nodes = n + (lead ? n_trees : 0);
  tmh::StageLayout L;
  const size_t o_gw = L.in(8ull * n), o_gu = L.in(8ull * n), o_code = L.in(4ull * n), o_doff = L.in(4ull * (n + 1ull));
  const size_t o_toff = L.in(4ull * (n_trees + 1ull)), o_noff = L.in(lead ? 4ull * (n_trees + 1ull) : 0);
  const size_t o_foff = L.in(lead ? 4ull * (n_trees + 1ull) : 0), o_data = L.in(bytes);
  const size_t o_first = lead ? L.in_padded(first_bytes) : 0;
  const size_t o_fn = L.scratch(lead ? 32ull * n_trees : 0);  // the leading leaves' nodes, before they are placed
  const size_t o_na = L.scratch(32ull * nodes), o_nb = L.scratch(32ull * nodes);  // two node arrays
  const size_t o_out = L.out(32ull * n_trees);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_gw, gas_wanted, 8ull * n);
  c.put(o_gu, gas_used, 8ull * n);
  c.put(o_code, code, 4ull * n);
  c.put(o_doff, data_off, n ? 4ull * (n + 1ull) : 0);  // without results nothing reads it
  c.put(o_toff, tree_off, 4ull * (n_trees + 1ull));
  c.put(o_data, data, bytes);
  if (lead) {
    uint32_t *noff = reinterpret_cast<uint32_t *>(c.h + o_noff);  // tree t's nodes: its leading leaf, then its results
    for (uint32_t t = 0; t <= n_trees; t++) noff[t] = tree_off[t] + t;
    c.put(o_foff, first_off, 4ull * (n_trees + 1ull));
    c.put(o_first, first, first_bytes);
  }
  if ((rc = c.upload("hipMemcpyAsync(tx results)")) != 0) return rc;
  hipError_t e = hipSuccess;
  if (lead)
    e = merkle_launch_leaves(kernel, 0, c.g + o_first, c.dev<const uint32_t>(o_foff), n_trees, c.dev<uint32_t>(o_fn),
                             c.s);
  if (e == hipSuccess)
    e = tmv::launch_results_hashes(c.dev<const uint32_t>(o_code), c.dev<const int64_t>(o_gw),
                                   c.dev<const int64_t>(o_gu), c.g + o_data, c.dev<const uint32_t>(o_doff), n,
                                   c.dev<const uint32_t>(o_toff), c.dev<const uint32_t>(lead ? o_noff : o_toff),
                                   n_trees, max_leaves + (lead ? 1 : 0), lead ? c.dev<const uint32_t>(o_fn) : nullptr,
                                   c.dev<uint32_t>(o_na), c.dev<uint32_t>(o_nb), c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("tx results launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("tx results readback", root_out, 32ull * n_trees);
}

}  // extern "C"
