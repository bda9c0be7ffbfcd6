// tmv_commit_hashes (include/tmverify.h): Commit.Hash (types/block.go:900-918)
// of many commits behind the C-ABI.  Kept out of tmverify_runtime.cpp, which
// includes this file at its end: the entry point shares its Device, staging
// buffers, bounded waits and error text.  Synchronous, host buffers, device 0;
// staged like tmv_validator_set_hashes: one H2D copy, the two launches
// (commit_kernels.hip), one D2H copy.
#pragma once
#include "commit_hash.h"

extern "C" {

int tmv_commit_hashes(tmv_ctx *ctx, const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                      const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len, const uint8_t *sig,
                      const uint32_t *commit_off, uint32_t n_commits, uint8_t *hash_out) {
  if (!ctx || ctx->devs.empty()) { set_error("null context"); return TMV_ERR_ARG; }
  if (n_commits == 0) return 0;
  if (!commit_off || !hash_out) { set_error("tmv_commit_hashes: null pointer"); return TMV_ERR_ARG; }
  if (commit_off[0] != 0) { set_error("tmv_commit_hashes: commit_off[0] must be 0"); return TMV_ERR_ARG; }
  uint32_t max_sigs = 0;
  for (uint32_t c = 0; c < n_commits; c++) {
    if (commit_off[c + 1] < commit_off[c]) { set_error("tmv_commit_hashes: commit_off decreasing"); return TMV_ERR_ARG; }
    max_sigs = std::max(max_sigs, commit_off[c + 1] - commit_off[c]);
  }
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
  Device &d = *ctx->devs[0];
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.faulted) return faulted_rc(d);
  hipError_t e = hipSetDevice(d.id);
  if (e != hipSuccess) { set_error("hipSetDevice", e); return TMV_ERR_NO_DEVICE; }
  // staging: sig | seconds | nanos | addr | commit_off | flag | addr_len | sig_len, then (device only) two
  // node arrays and the roots
  const size_t o_sec = 64ull * n, o_nan = o_sec + align16(8ull * n), o_addr = o_nan + align16(4ull * n);
  const size_t o_off = o_addr + align16(20ull * n), o_flag = o_off + align16(4ull * (n_commits + 1));
  const size_t o_alen = o_flag + align16(n), o_slen = o_alen + align16(n), in_bytes = o_slen + align16(n);
  const size_t o_na = in_bytes, o_nb = o_na + 32ull * n, o_out = o_nb + 32ull * n;
  const size_t dev_bytes = o_out + 32ull * n_commits;
  hipStream_t s = context_stream(d);
  if (!s) { set_error("hipStreamCreate failed"); return TMV_ERR_NO_DEVICE; }
  if ((e = wait_stream(d, s)) != hipSuccess) return wait_rc(e);  // staging shared with tmv_validator_set_hashes
  if ((e = d.h_valset.ensure(in_bytes, true)) != hipSuccess) { set_error("hipHostMalloc", e); return TMV_ERR_NOMEM; }
  if ((e = d.d_valset.ensure(dev_bytes, false)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
  uint8_t *h = static_cast<uint8_t *>(d.h_valset.ptr);
  if (n) {
    std::memcpy(h, sig, 64ull * n);
    std::memcpy(h + o_sec, ts_seconds, 8ull * n);
    std::memcpy(h + o_nan, ts_nanos, 4ull * n);
    std::memcpy(h + o_addr, addr, 20ull * n);
    std::memcpy(h + o_flag, flag, n);
    std::memcpy(h + o_alen, addr_len, n);
    std::memcpy(h + o_slen, sig_len, n);
  }
  std::memcpy(h + o_off, commit_off, 4ull * (n_commits + 1));
  uint8_t *g = static_cast<uint8_t *>(d.d_valset.ptr);
  if ((e = hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) {
    set_error("hipMemcpyAsync(commit hashes)", e);
    return TMV_ERR_LAUNCH;
  }
  e = tmv::launch_commit_hashes(g + o_flag, g + o_alen, g + o_addr, reinterpret_cast<const int64_t *>(g + o_sec),
                                reinterpret_cast<const int32_t *>(g + o_nan), g + o_slen, g, n,
                                reinterpret_cast<const uint32_t *>(g + o_off), n_commits, max_sigs,
                                reinterpret_cast<uint32_t *>(g + o_na), reinterpret_cast<uint32_t *>(g + o_nb),
                                g + o_out, s);
  if (e != hipSuccess) { set_error("commit hash launch", e); return TMV_ERR_LAUNCH; }
  if ((e = hipMemcpyAsync(hash_out, g + o_out, 32ull * n_commits, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = wait_stream(d, s)) != hipSuccess) {
    if (e != hipErrorNotReady) set_error("commit hash readback", e);
    return wait_rc(e);
  }
  return 0;
}

}  // extern "C"
