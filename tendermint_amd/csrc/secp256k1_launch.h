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

// ---- cached keys (secp256k1.h, comb tables) ----
// A key's slot is secp256k1_comb_bytes() of `table`; an entry whose key cannot
// have one carries kSecpNoSlot.
constexpr uint32_t kSecpNoSlot = 0xFFFFFFFFu;
size_t secp256k1_comb_bytes();
// Workspace of one cached launch of n entries: a 128-byte record per entry.
size_t secp256k1_cached_workspace_bytes(uint32_t n);

// Builds the combs of n_keys keys (pk48: 48-byte stride) into table slots
// slot[k] (each below the table's capacity; distinct).  slot_ok[slot[k]] and
// miss_ok[k] <- 1 if key k parsed, else 0 (the slot then holds G's comb).
hipError_t launch_secp256k1_key_tables(const uint8_t *pk48, const uint32_t *slot, uint32_t n_keys, uint32_t *table,
                                       uint32_t *slot_ok, uint32_t *miss_ok, hipStream_t stream);

// As launch_secp256k1_verify with slot[i] (a built slot or kSecpNoSlot) in
// place of the keys; gcomb: G's comb (secp::build_comb); work:
// secp256k1_cached_workspace_bytes(n), 256-byte aligned.
hipError_t launch_secp256k1_verify_cached(const uint8_t *sig, const uint8_t *msg, const uint32_t *msg_off,
                                          const uint32_t *slot, uint32_t n, const uint32_t *gcomb,
                                          const uint32_t *table, const uint32_t *slot_ok, uint8_t *work,
                                          uint8_t *valid, hipStream_t stream);

}  // namespace tmv
