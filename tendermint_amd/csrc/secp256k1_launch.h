// secp256k1 ECDSA verification (secp256k1_kernels.hip): launch wrapper shared
// with the runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tmv {

// Workspace of one launch of n entries: a 128-byte record and a 2,048-byte
// table of Q multiples per entry.
size_t secp256k1_workspace_bytes(uint32_t n);

// pk48: n keys at a 48-byte stride (33 bytes each, 16-byte aligned); sig: n x
// 64 bytes (16-byte aligned); msg_off: n + 1 offsets into msg; gtab: the G
// table (secp::build_g_table); work: secp256k1_workspace_bytes(n), 256-byte
// aligned; valid: n bytes, 1 / 0.
hipError_t launch_secp256k1_verify(const uint8_t *pk48, const uint8_t *sig, const uint8_t *msg,
                                   const uint32_t *msg_off, uint32_t n, const uint32_t *gtab, uint8_t *work,
                                   uint8_t *valid, hipStream_t stream);

}  // namespace tmv
