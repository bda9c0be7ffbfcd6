// C entry point over csrc/host/results_encode.h for tests/test_results_host.py:
// the protobuf bytes of one tx result as the host layer encodes them.
#include <cstring>

#include "host/results_encode.h"

extern "C" {

// Returns the length; writes min(length, cap) bytes.
size_t rs_tx_result_encode(const tmv_tx_result *r, uint8_t *out, size_t cap) {
  tmh::Bytes b;
  tmh::AppendTxResultProto(*r, b);
  if (!b.empty()) std::memcpy(out, b.data(), b.size() < cap ? b.size() : cap);
  return b.size();
}

}  // extern "C"
