// C entry point over csrc/host/commit_encode.h for tests/test_blocks_host.py:
// the protobuf bytes of one CommitSig as the host layer encodes them.
#include <cstring>

#include "host/commit_encode.h"

extern "C" {

// Returns the length; writes min(length, cap) bytes.
size_t bk_commit_sig_encode(const tmv_commit_sig *s, uint8_t *out, size_t cap) {
  tmh::Bytes b;
  tmh::AppendCommitSigProto(*s, b);
  if (!b.empty()) std::memcpy(out, b.data(), b.size() < cap ? b.size() : cap);
  return b.size();
}

}  // extern "C"
