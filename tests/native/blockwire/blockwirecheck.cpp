// C entry point over csrc/host/block_wire.h for tests/test_block_wire_host.py:
// the span table the scanner makes of one block, in the order the host layer
// hands it to the engine.
#include <cstring>

#include "host/block_wire.h"

extern "C" {

// Scans data[0, len).  Returns the reason; on 0 writes min(count, cap) spans --
// the commit-signature leaves, the transaction leaves, the 14 header leaves --
// and their three counts.
int bw_block_spans(const uint8_t *data, uint32_t len, tmv_leaf_span *out, uint32_t cap, uint32_t counts[3]) {
  tmw::BlockScan s;
  const tmw::Reason r = tmw::scan_block(data, 0, len, s);
  if (r != tmw::kNone) return r;
  counts[0] = (uint32_t)s.sig_leaf.size();
  counts[1] = (uint32_t)s.tx_leaf.size();
  counts[2] = tmw::kHeaderLeaves;
  uint32_t k = 0;
  auto emit = [&](const tmv_leaf_span &l) {
    if (k < cap) out[k] = l;
    k++;
  };
  for (const tmv_leaf_span &l : s.sig_leaf) emit(l);
  for (const tmv_leaf_span &l : s.tx_leaf) emit(l);
  for (const tmv_leaf_span &l : s.hdr_leaf) emit(l);
  return 0;
}

}  // extern "C"
