// Device Commit.Hash (commit_kernels.hip): launch wrapper shared with the
// runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmv {

// Commit.Hash (types/block.go:900-918) of n_commits commits: commit c holds
// the signatures [commit_off[c], commit_off[c+1]) of the column arrays (all
// device pointers; addr 4-byte and sig 16-byte aligned) and at most max_sigs
// of them.  The caller has checked flag <= 127, addr_len in {0, 20} and
// sig_len <= 64.  node_a / node_b: n_sigs x 8 words each; out: n_commits x 32 B.
hipError_t launch_commit_hashes(const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                                const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len,
                                const uint8_t *sig, uint32_t n_sigs, const uint32_t *commit_off, uint32_t n_commits,
                                uint32_t max_sigs, uint32_t *node_a, uint32_t *node_b, uint8_t *out,
                                hipStream_t stream);

}  // namespace tmv
