// Chained value proof operators (merkle_ops_kernels.hip): the launch wrapper
// shared with the runtime (merkle_ops_runtime.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmv {

// ValueOp.Run chained per item: item i owns ops [op_off[i], op_off[i+1]);
// vdig holds the 8 state words of SHA-256(value_i).  Hash arrays are 16-byte
// aligned; outputs as tmv_merkle_value_ops (include/tmverify.h).
hipError_t launch_merkle_value_ops(uint32_t n_items, const uint32_t *op_off, const uint32_t *vdig, const uint8_t *key,
                                   const uint32_t *key_off, const int64_t *total, const int64_t *index,
                                   const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                                   const uint8_t *root, uint8_t *kv_out, uint8_t *leaf_ok_out, uint8_t *rootc_out,
                                   uint8_t *nil_out, int8_t *status_out, int32_t *fail_op_out, hipStream_t stream);

}  // namespace tmv
