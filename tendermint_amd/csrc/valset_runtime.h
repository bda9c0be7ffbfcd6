// tmv_validator_set_hashes (include/tmverify.h): ValidatorSet.Hash of many
// sets in one launch (types/validator_set.go:344-350)
// behind the C-ABI.  Included by tmverify_runtime.cpp at its end.  A staged
// call (staged_call.h) with the kernels of merkle_kernels.hip.
#pragma once
#include "valset.h"

extern "C" {

int tmv_validator_set_hashes(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *key_kind, const int64_t *power,
                             const uint32_t *set_off, uint32_t n_sets, uint8_t *hash_out) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_sets == 0) return 0;
  if (!set_off || !hash_out) { set_error("tmv_validator_set_hashes: null pointer"); return TMV_ERR_ARG; }
  if ((rc = offsets_rc("tmv_validator_set_hashes", "set_off", set_off, n_sets)) != 0) return rc;
  const uint32_t n = set_off[n_sets];
  if (n && (!pk || !key_kind || !power)) { set_error("tmv_validator_set_hashes: null pointer"); return TMV_ERR_ARG; }
  if (n > (1u << 26)) { set_error("tmv_validator_set_hashes: too many validators"); return TMV_ERR_ARG; }
  for (uint32_t i = 0; i < n; i++)
    if (key_kind[i] != TMV_KIND_ED25519 && key_kind[i] != TMV_KIND_SR25519) {
      set_error("tmv_validator_set_hashes: key kind must be ed25519 or sr25519");
      return TMV_ERR_ARG;
    }
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_power = L.in(8ull * n), o_off = L.in(4ull * (n_sets + 1)), o_pk = L.in(32ull * n), o_kind = L.in(n);
  const size_t o_na = L.scratch(32ull * n), o_nb = L.scratch(32ull * n);  // two node arrays
  const size_t o_out = L.out(32ull * n_sets);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_power, power, 8ull * n);
  c.put(o_off, set_off, 4ull * (n_sets + 1));
  c.put(o_pk, pk, 32ull * n);
  c.put(o_kind, key_kind, n);
  if ((rc = c.upload("hipMemcpyAsync(valset)")) != 0) return rc;
  const hipError_t e = tmv::launch_valset_hashes(c.g + o_pk, c.g + o_kind, c.dev<const int64_t>(o_power), n,
                                                 c.dev<const uint32_t>(o_off), n_sets, c.dev<uint32_t>(o_na),
                                                 c.dev<uint32_t>(o_nb), c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("valset hash launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("valset hash readback", hash_out, 32ull * n_sets);
}

}  // extern "C"
