// tmv_merkle_value_ops (include/tmverify.h): ValueOp.Run (crypto/merkle/
// proof_value.go:77-98) chained as ProofOperators.Verify chains it
// (proof_op.go:39-69) behind the C-ABI.  Included by tmverify_runtime.cpp after
// merkle_runtime.h, whose staging (d.h_valset / d.d_valset), leaves-per-wave
// choice and padding it reuses.  Synchronous, host buffers, device 0: one H2D
// copy, k_merkle_digests_long and k_merkle_value_ops, one D2H copy.
#pragma once
#include "merkle_ops.h"
#include "merkle_proof.h"

namespace {

int value_ops_offsets(const char *what, const uint32_t *off, uint32_t n) {
  const std::string w = std::string("tmv_merkle_value_ops: ") + what;
  if (off[0] != 0) { set_error(w + "[0] must be 0"); return TMV_ERR_ARG; }
  for (uint32_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) { set_error(w + " decreasing"); return TMV_ERR_ARG; }
  return 0;
}

}  // namespace

extern "C" {

int tmv_merkle_value_ops(tmv_ctx *ctx, uint32_t flags, uint32_t n_items, const uint8_t *value,
                         const uint32_t *value_off, const uint32_t *op_off, const uint8_t *key, const uint32_t *key_off,
                         const int64_t *total, const int64_t *index, const uint8_t *leaf_hash, const uint8_t *aunts,
                         const uint32_t *aunt_off, const uint8_t *root, uint8_t *value_digest, uint8_t *kv_hash_calc,
                         uint8_t *leaf_ok, uint8_t *root_calc, uint8_t *root_nil, int8_t *status_out,
                         int32_t *fail_op_out) {
  if (!ctx || ctx->devs.empty()) { set_error("null context"); return TMV_ERR_ARG; }
  if (n_items == 0) return 0;
  if (!value_off || !op_off || !key_off || !total || !index || !leaf_hash || !aunt_off || !root) {
    set_error("tmv_merkle_value_ops: null pointer");
    return TMV_ERR_ARG;
  }
  if (n_items > (1u << 26)) { set_error("tmv_merkle_value_ops: input too large"); return TMV_ERR_ARG; }
  int rc = value_ops_offsets("value_off", value_off, n_items);
  if (rc == 0) rc = value_ops_offsets("op_off", op_off, n_items);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (op_off[i + 1] == op_off[i]) { set_error("tmv_merkle_value_ops: an item without ops"); return TMV_ERR_ARG; }
  const uint32_t n_ops = op_off[n_items];
  if (n_ops > (1u << 26)) { set_error("tmv_merkle_value_ops: input too large"); return TMV_ERR_ARG; }
  if ((rc = value_ops_offsets("key_off", key_off, n_ops)) != 0) return rc;
  if ((rc = value_ops_offsets("aunt_off", aunt_off, n_ops)) != 0) return rc;
  const uint32_t vbytes = value_off[n_items], kbytes = key_off[n_ops], n_aunts = aunt_off[n_ops];
  if (vbytes > (1u << 30) || kbytes > (1u << 30) || n_aunts > (1u << 28)) {
    set_error("tmv_merkle_value_ops: input too large");
    return TMV_ERR_ARG;
  }
  if ((vbytes && !value) || (kbytes && !key) || (n_aunts && !aunts)) {
    set_error("tmv_merkle_value_ops: null data");
    return TMV_ERR_ARG;
  }
  const uint32_t lpw_flag = (flags >> 8) & 0xff;
  if ((flags & 0xff) || (flags >> 16) || (lpw_flag && lpw_flag != 8 && lpw_flag != 16 && lpw_flag != 32 && lpw_flag != 64)) {
    set_error("tmv_merkle_value_ops: bad flags");
    return TMV_ERR_ARG;
  }
  const uint32_t lpw = lpw_flag ? lpw_flag : tmh::merkle_leaves_per_wave(n_items);
  Device &d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.faulted) return faulted_rc(d);
  hipError_t e = hipSetDevice(d.id);
  if (e != hipSuccess) { set_error("hipSetDevice", e); return TMV_ERR_NO_DEVICE; }
  // staging: total | index | leaf hashes | roots | aunts | aunt_off | op_off | key_off | value_off | keys |
  // 16 bytes of padding | values, then (device only) the value digests and the outputs
  // kv hashes | roots | value digests | leaf_ok | nil flags | statuses | failing ops
  const size_t o_index = 8ull * n_ops, o_lh = 2 * o_index, o_root = o_lh + 32ull * n_ops;
  const size_t o_aunts = o_root + 32ull * n_items, o_aoff = o_aunts + 32ull * n_aunts;
  const size_t o_ooff = o_aoff + align16(4ull * (n_ops + 1)), o_koff = o_ooff + align16(4ull * (n_items + 1));
  const size_t o_voff = o_koff + align16(4ull * (n_ops + 1)), o_keys = o_voff + align16(4ull * (n_items + 1));
  const size_t o_val = o_keys + align16(kbytes) + 16;
  const size_t in_bytes = o_val + align16(vbytes);
  const size_t o_out = in_bytes;
  const size_t q_rootc = 32ull * n_ops, q_vdig = 2 * q_rootc, q_lok = q_vdig + 32ull * n_items;
  const size_t q_nil = q_lok + align16(n_ops), q_status = q_nil + align16(n_ops), q_fail = q_status + align16(n_items);
  const size_t out_bytes = q_fail + align16(4ull * n_items);
  hipStream_t s = context_stream(d);
  if (!s) { set_error("hipStreamCreate failed"); return TMV_ERR_NO_DEVICE; }
  if ((e = wait_stream(d, s)) != hipSuccess) return wait_rc(e);  // staging shared with tmv_merkle_roots
  if ((e = d.h_valset.ensure(std::max(in_bytes, out_bytes), true)) != hipSuccess) {
    set_error("hipHostMalloc", e);
    return TMV_ERR_NOMEM;
  }
  if ((e = d.d_valset.ensure(o_out + out_bytes, false)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
  uint8_t *h = static_cast<uint8_t *>(d.h_valset.ptr);
  std::memcpy(h, total, 8ull * n_ops);
  std::memcpy(h + o_index, index, 8ull * n_ops);
  std::memcpy(h + o_lh, leaf_hash, 32ull * n_ops);
  std::memcpy(h + o_root, root, 32ull * n_items);
  if (n_aunts) std::memcpy(h + o_aunts, aunts, 32ull * n_aunts);
  std::memcpy(h + o_aoff, aunt_off, 4ull * (n_ops + 1));
  std::memcpy(h + o_ooff, op_off, 4ull * (n_items + 1));
  std::memcpy(h + o_koff, key_off, 4ull * (n_ops + 1));
  std::memcpy(h + o_voff, value_off, 4ull * (n_items + 1));
  if (kbytes) std::memcpy(h + o_keys, key, kbytes);
  std::memset(h + o_val - 16, 0, 16);
  if (vbytes) std::memcpy(h + o_val, value, vbytes);
  uint8_t *g = static_cast<uint8_t *>(d.d_valset.ptr);
  if ((e = hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) {
    set_error("hipMemcpyAsync(merkle value ops)", e);
    return TMV_ERR_LAUNCH;
  }
  uint8_t *go = g + o_out;
  uint32_t *vdig = reinterpret_cast<uint32_t *>(go + q_vdig);
  e = tmv::launch_merkle_digests_long(g + o_val, reinterpret_cast<const uint32_t *>(g + o_voff), n_items, lpw, vdig, s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_value_ops(n_items, reinterpret_cast<const uint32_t *>(g + o_ooff), vdig, g + o_keys,
                                     reinterpret_cast<const uint32_t *>(g + o_koff),
                                     reinterpret_cast<const int64_t *>(g), reinterpret_cast<const int64_t *>(g + o_index),
                                     g + o_lh, g + o_aunts, reinterpret_cast<const uint32_t *>(g + o_aoff), g + o_root,
                                     go, go + q_lok, go + q_rootc, go + q_nil,
                                     reinterpret_cast<int8_t *>(go + q_status),
                                     reinterpret_cast<int32_t *>(go + q_fail), s);
  if (e != hipSuccess) { set_error("merkle value ops launch", e); return TMV_ERR_LAUNCH; }
  if ((e = hipMemcpyAsync(h, go, out_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = wait_stream(d, s)) != hipSuccess) {
    if (e != hipErrorNotReady) set_error("merkle value ops readback", e);
    return wait_rc(e);
  }
  if (kv_hash_calc) std::memcpy(kv_hash_calc, h, 32ull * n_ops);
  if (root_calc) std::memcpy(root_calc, h + q_rootc, 32ull * n_ops);
  if (value_digest) {  // the state words, serialised big-endian
    const uint32_t *w = reinterpret_cast<const uint32_t *>(h + q_vdig);
    for (size_t k = 0; k < 8ull * n_items; k++)
      for (int b = 0; b < 4; b++) value_digest[4 * k + b] = (uint8_t)(w[k] >> (24 - 8 * b));
  }
  if (leaf_ok) std::memcpy(leaf_ok, h + q_lok, n_ops);
  if (root_nil) std::memcpy(root_nil, h + q_nil, n_ops);
  const int8_t *st = reinterpret_cast<const int8_t *>(h + q_status);
  if (status_out) std::memcpy(status_out, st, n_items);
  if (fail_op_out) std::memcpy(fail_op_out, h + q_fail, 4ull * n_items);
  bool all = true;
  for (uint32_t i = 0; i < n_items; i++) all = all && st[i] == 0;
  return all ? 0 : 1;
}

}  // extern "C"
