// Where the regions of one staged call sit (staged_call.h; DESIGN.md "Staged
// calls"): the inputs, copied to the device in one piece; scratch that only the
// device sees; the outputs, copied back in one piece.  Regions are handed out
// in that order, each from the next 16-byte boundary, so they cannot overlap.
// Pure host arithmetic with no HIP in it, unit-tested on the CPU
// (tests/test_stage_layout.py through tests/native/stage/).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)  // header-only: adds nothing to a library's exported symbols
namespace tmh {

inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

struct StageLayout {
  size_t in_bytes = 0;   // [0, in_bytes) is copied to the device
  size_t out_at = 0;     // [out_at, out_at + out_bytes) is copied back
  size_t out_bytes = 0;
  size_t dev_bytes = 0;  // the device buffer: inputs, scratch, outputs
  size_t pad_at = 0;     // in_padded's region (0: none); the 16 bytes before it are staged as zeros

  // Every call returns its region's offset in the device buffer (inputs: in
  // the pinned buffer as well).  spare: bytes behind the region a kernel may
  // read, kept inside it.
  size_t in(size_t bytes, size_t spare = 0) {
    assert(phase_ == 0);
    const size_t at = take(bytes + spare);
    in_bytes = out_at = dev_bytes;
    return at;
  }
  // An input with 16 zero bytes in front of it, which k_merkle_leaves_long and
  // k_merkle_digests_long read ahead of a region's first unit.
  size_t in_padded(size_t bytes) {
    assert(phase_ == 0 && pad_at == 0);
    dev_bytes += 16;
    return pad_at = in(bytes);
  }
  size_t scratch(size_t bytes) {
    assert(phase_ <= 1);
    phase_ = 1;
    const size_t at = take(bytes);
    out_at = dev_bytes;
    return at;
  }
  size_t out(size_t bytes) {
    phase_ = 2;
    const size_t at = take(bytes);
    out_bytes = dev_bytes - out_at;
    return at;
  }

 private:
  int phase_ = 0;  // 0 inputs, 1 scratch, 2 outputs: never back
  size_t take(size_t bytes) {
    const size_t at = dev_bytes;
    dev_bytes += align16(bytes);
    return at;
  }
};

// Prefix offsets off[0..n]: must start at 0 and never decrease.  *max_span
// (may be null): the largest off[i + 1] - off[i], 0 for n == 0.
enum class Offsets { kOk, kFirstNotZero, kDecreasing };
inline Offsets check_offsets(const uint32_t *off, uint32_t n, uint32_t *max_span) {
  if (off[0] != 0) return Offsets::kFirstNotZero;
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (off[i + 1] < off[i]) return Offsets::kDecreasing;
    if (off[i + 1] - off[i] > m) m = off[i + 1] - off[i];
  }
  if (max_span) *max_span = m;
  return Offsets::kOk;
}

}  // namespace tmh
#pragma GCC visibility pop
