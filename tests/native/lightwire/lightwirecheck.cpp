// C entry point over csrc/host/light_wire.h for tests/test_light_wire_host.py:
// the span tables the scanner makes of one light block, as the host layer
// hands them to the engine.
#include <cstring>

#include "host/light_wire.h"

extern "C" {

// Scans data[0, len).  Returns the reason; on 0 writes the 14 header leaves to
// hdr_out (zeros without a header) and min(count, cap) validator spans to
// val_out, and *n_vals = their count.
int lw_light_block_spans(const uint8_t *data, uint32_t len, tmv_leaf_span *hdr_out, tmv_val_span *val_out, uint32_t cap,
                         uint32_t *n_vals) {
  tmw::LightScan s;
  const tmw::Reason r = tmw::scan_light_block(data, 0, len, s);
  if (r != tmw::kNone) return r;
  std::memcpy(hdr_out, s.b.hdr_leaf, sizeof s.b.hdr_leaf);
  *n_vals = (uint32_t)s.val_leaf.size();
  for (uint32_t k = 0; k < s.val_leaf.size() && k < cap; k++) val_out[k] = s.val_leaf[k];
  return 0;
}

}  // extern "C"
