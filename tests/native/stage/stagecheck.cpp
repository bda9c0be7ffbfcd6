// C entry points over csrc/host/stage_layout.h for tests/test_stage_layout.py.
#include "host/stage_layout.h"

extern "C" {

// kind[i]: 0 in (with spare[i]), 1 in_padded, 2 scratch, 3 out.  at_out: n offsets;
// spans_out: in_bytes, out_at, out_bytes, dev_bytes, pad_at.
void sl_layout(const uint8_t *kind, const uint64_t *bytes, const uint64_t *spare, uint32_t n, uint64_t *at_out,
               uint64_t *spans_out) {
  tmh::StageLayout L;
  for (uint32_t i = 0; i < n; i++)
    at_out[i] = kind[i] == 0 ? L.in(bytes[i], spare[i]) : kind[i] == 1 ? L.in_padded(bytes[i])
              : kind[i] == 2 ? L.scratch(bytes[i]) : L.out(bytes[i]);
  const uint64_t spans[5] = {L.in_bytes, L.out_at, L.out_bytes, L.dev_bytes, L.pad_at};
  for (int k = 0; k < 5; k++) spans_out[k] = spans[k];
}

// 0 ok, 1 first not zero, 2 decreasing.
int sl_check_offsets(const uint32_t *off, uint32_t n, uint32_t *max_span) {
  return (int)tmh::check_offsets(off, n, max_span);
}

}  // extern "C"
