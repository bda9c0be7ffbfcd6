// tmv_merkle_value_ops (include/tmverify.h): ValueOp.Run (crypto/merkle/
// proof_value.go:77-98) chained as ProofOperators.Verify chains it
// (proof_op.go:39-69) behind the C-ABI.  Included by tmverify_runtime.cpp after
// merkle_runtime.h, whose leaves-per-wave choice it reuses.  A staged call
// (staged_call.h) with k_merkle_digests_long and k_merkle_value_ops.
#pragma once
#include "merkle_ops.h"
#include "merkle_proof.h"

extern "C" {

int tmv_merkle_value_ops(tmv_ctx *ctx, uint32_t flags, uint32_t n_items, const uint8_t *value,
                         const uint32_t *value_off, const uint32_t *op_off, const uint8_t *key, const uint32_t *key_off,
                         const int64_t *total, const int64_t *index, const uint8_t *leaf_hash, const uint8_t *aunts,
                         const uint32_t *aunt_off, const uint8_t *root, uint8_t *value_digest, uint8_t *kv_hash_calc,
                         uint8_t *leaf_ok, uint8_t *root_calc, uint8_t *root_nil, int8_t *status_out,
                         int32_t *fail_op_out) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_items == 0) return 0;
  if (!value_off || !op_off || !key_off || !total || !index || !leaf_hash || !aunt_off || !root) {
    set_error("tmv_merkle_value_ops: null pointer");
    return TMV_ERR_ARG;
  }
  if (n_items > (1u << 26)) { set_error("tmv_merkle_value_ops: input too large"); return TMV_ERR_ARG; }
  const char *fn = "tmv_merkle_value_ops";
  if ((rc = offsets_rc(fn, "value_off", value_off, n_items)) != 0) return rc;
  if ((rc = offsets_rc(fn, "op_off", op_off, n_items)) != 0) return rc;
  for (uint32_t i = 0; i < n_items; i++)
    if (op_off[i + 1] == op_off[i]) { set_error("tmv_merkle_value_ops: an item without ops"); return TMV_ERR_ARG; }
  const uint32_t n_ops = op_off[n_items];
  if (n_ops > (1u << 26)) { set_error("tmv_merkle_value_ops: input too large"); return TMV_ERR_ARG; }
  if ((rc = offsets_rc(fn, "key_off", key_off, n_ops)) != 0) return rc;
  if ((rc = offsets_rc(fn, "aunt_off", aunt_off, n_ops)) != 0) return rc;
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
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_total = L.in(8ull * n_ops), o_index = L.in(8ull * n_ops), o_lh = L.in(32ull * n_ops);
  const size_t o_root = L.in(32ull * n_items), o_aunts = L.in(32ull * n_aunts), o_aoff = L.in(4ull * (n_ops + 1));
  const size_t o_ooff = L.in(4ull * (n_items + 1)), o_koff = L.in(4ull * (n_ops + 1));
  const size_t o_voff = L.in(4ull * (n_items + 1)), o_keys = L.in(kbytes), o_val = L.in_padded(vbytes);
  const size_t q_kv = L.out(32ull * n_ops), q_rootc = L.out(32ull * n_ops), q_vdig = L.out(32ull * n_items);
  const size_t q_lok = L.out(n_ops), q_nil = L.out(n_ops), q_status = L.out(n_items), q_fail = L.out(4ull * n_items);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, true)) != 0) return rc;
  c.put(o_total, total, 8ull * n_ops);
  c.put(o_index, index, 8ull * n_ops);
  c.put(o_lh, leaf_hash, 32ull * n_ops);
  c.put(o_root, root, 32ull * n_items);
  c.put(o_aunts, aunts, 32ull * n_aunts);
  c.put(o_aoff, aunt_off, 4ull * (n_ops + 1));
  c.put(o_ooff, op_off, 4ull * (n_items + 1));
  c.put(o_koff, key_off, 4ull * (n_ops + 1));
  c.put(o_voff, value_off, 4ull * (n_items + 1));
  c.put(o_keys, key, kbytes);
  c.put(o_val, value, vbytes);
  if ((rc = c.upload("hipMemcpyAsync(merkle value ops)")) != 0) return rc;
  uint32_t *vdig = c.dev<uint32_t>(q_vdig);
  hipError_t e = tmv::launch_merkle_digests_long(c.g + o_val, c.dev<const uint32_t>(o_voff), n_items, lpw, vdig, c.s);
  if (e == hipSuccess)
    e = tmv::launch_merkle_value_ops(n_items, c.dev<const uint32_t>(o_ooff), vdig, c.g + o_keys,
                                     c.dev<const uint32_t>(o_koff), c.dev<const int64_t>(o_total),
                                     c.dev<const int64_t>(o_index), c.g + o_lh, c.g + o_aunts,
                                     c.dev<const uint32_t>(o_aoff), c.g + o_root, c.g + q_kv, c.g + q_lok, c.g + q_rootc,
                                     c.g + q_nil, c.dev<int8_t>(q_status), c.dev<int32_t>(q_fail), c.s);
  if (e != hipSuccess) { set_error("merkle value ops launch", e); return TMV_ERR_LAUNCH; }
  if ((rc = c.finish("merkle value ops readback")) != 0) return rc;
  if (kv_hash_calc) std::memcpy(kv_hash_calc, c.result(q_kv), 32ull * n_ops);
  if (root_calc) std::memcpy(root_calc, c.result(q_rootc), 32ull * n_ops);
  if (value_digest) {  // the state words, serialised big-endian
    const uint32_t *w = reinterpret_cast<const uint32_t *>(c.result(q_vdig));
    for (size_t k = 0; k < 8ull * n_items; k++)
      for (int b = 0; b < 4; b++) value_digest[4 * k + b] = (uint8_t)(w[k] >> (24 - 8 * b));
  }
  if (leaf_ok) std::memcpy(leaf_ok, c.result(q_lok), n_ops);
  if (root_nil) std::memcpy(root_nil, c.result(q_nil), n_ops);
  const int8_t *st = reinterpret_cast<const int8_t *>(c.result(q_status));
  if (status_out) std::memcpy(status_out, st, n_items);
  if (fail_op_out) std::memcpy(fail_op_out, c.result(q_fail), 4ull * n_items);
  bool all = true;
  for (uint32_t i = 0; i < n_items; i++) all = all && st[i] == 0;
  return all ? 0 : 1;
}

}  // extern "C"
