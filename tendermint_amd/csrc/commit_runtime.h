// tmv_commit_hashes (include/tmverify.h): Commit.Hash (types/block.go:900-918)
// of many commits behind the C-ABI.  Kept out of tmverify_runtime.cpp, which
// includes this file at its end.  A staged call (staged_call.h) with the two
// launches of commit_kernels.hip.
#pragma once
#include "commit_hash.h"

extern "C" {

int tmv_commit_hashes(tmv_ctx *ctx, const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                      const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len, const uint8_t *sig,
                      const uint32_t *commit_off, uint32_t n_commits, uint8_t *hash_out) {
  StagedCall c;
  int rc = c.attach(ctx);
  if (rc) return rc;
  if (n_commits == 0) return 0;
  if (!commit_off || !hash_out) { set_error("tmv_commit_hashes: null pointer"); return TMV_ERR_ARG; }
  uint32_t max_sigs = 0;
  if ((rc = offsets_rc("tmv_commit_hashes", "commit_off", commit_off, n_commits, &max_sigs)) != 0) return rc;
  const uint32_t n = commit_off[n_commits];
  if (n && (!flag || !addr_len || !addr || !ts_seconds || !ts_nanos || !sig_len || !sig)) {
    set_error("tmv_commit_hashes: null pointer");
    return TMV_ERR_ARG;
  }
  if (n > (1u << 26)) { set_error("tmv_commit_hashes: too many signatures"); return TMV_ERR_ARG; }
  for (uint32_t i = 0; i < n; i++) {
    if (flag[i] > 127) { set_error("tmv_commit_hashes: flag must be at most 127"); return TMV_ERR_ARG; }
    if (addr_len[i] != 0 && addr_len[i] != 20) { set_error("tmv_commit_hashes: addr_len must be 0 or 20"); return TMV_ERR_ARG; }
    if (sig_len[i] > 64) { set_error("tmv_commit_hashes: sig_len must be at most 64"); return TMV_ERR_ARG; }
  }
  if ((rc = c.open()) != 0) return rc;
  tmh::StageLayout L;
  const size_t o_sig = L.in(64ull * n), o_sec = L.in(8ull * n), o_nan = L.in(4ull * n), o_addr = L.in(20ull * n);
  const size_t o_off = L.in(4ull * (n_commits + 1)), o_flag = L.in(n), o_alen = L.in(n), o_slen = L.in(n);
  const size_t o_na = L.scratch(32ull * n), o_nb = L.scratch(32ull * n);  // two node arrays
  const size_t o_out = L.out(32ull * n_commits);
  if ((rc = c.reserve(L, c.d->h_stage, c.d->d_stage, false)) != 0) return rc;
  c.put(o_sig, sig, 64ull * n);
  c.put(o_sec, ts_seconds, 8ull * n);
  c.put(o_nan, ts_nanos, 4ull * n);
  c.put(o_addr, addr, 20ull * n);
  c.put(o_off, commit_off, 4ull * (n_commits + 1));
  c.put(o_flag, flag, n);
  c.put(o_alen, addr_len, n);
  c.put(o_slen, sig_len, n);
  if ((rc = c.upload("hipMemcpyAsync(commit hashes)")) != 0) return rc;
  const hipError_t e = tmv::launch_commit_hashes(
      c.g + o_flag, c.g + o_alen, c.g + o_addr, c.dev<const int64_t>(o_sec), c.dev<const int32_t>(o_nan), c.g + o_slen,
      c.g + o_sig, n, c.dev<const uint32_t>(o_off), n_commits, max_sigs, c.dev<uint32_t>(o_na), c.dev<uint32_t>(o_nb),
      c.g + o_out, c.s);
  if (e != hipSuccess) { set_error("commit hash launch", e); return TMV_ERR_LAUNCH; }
  return c.finish("commit hash readback", hash_out, 32ull * n_commits);
}

}  // extern "C"
