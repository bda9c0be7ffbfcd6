// Split key scalars of the batch equation (msm.h, "Split key scalars").
//
// With Ws = ceil(W / 2) and any scalar a and point P,
//   [a]P = [a mod 2^(c Ws)]P + [a >> (c Ws)]([2^(c Ws)]P).
// In signed c-bit digits d_w (sum d_w 2^(c w) = a) that is a relabelling of
// the recoding k_msm_sort already does: digit d_w with w < Ws stays the entry
// (window w, point P), digit d_w with w >= Ws becomes the entry
// (window w - Ws, point P_hi = [2^(c Ws)]P).  The digits themselves, and so
// the number of bucket entries, do not change; W - Ws <= Ws, so a group whose
// A and B scalars are relabelled this way uses windows [0, Ws) for them.
//
// Compiled for the device (msm_kernels.hip) and, unchanged, for the host
// (tests/native/split/).
#pragma once
#include <stdint.h>
#include "curve25519.h"  // TMV_HD

namespace tmv {

// Windows of a scalar's low half.
TMV_HD uint32_t split_windows(uint32_t W) { return (W + 1) / 2; }

// Where digit window w of an A or B scalar goes.
struct SplitSlot {
  uint32_t window;  // the bucket window
  uint32_t hi;      // 1: against the high point [2^(c Ws)]P, 0: against P
};
TMV_HD SplitSlot split_slot(uint32_t w, uint32_t Ws, bool split) {
  SplitSlot s;
  s.hi = split && w >= Ws ? 1u : 0u;
  s.window = s.hi ? w - Ws : w;
  return s;
}

// The most leaders a split group may have: one window of a split group
// stages its m R digits, a low and a high digit per leader and two B digits
// in the 2m + 1 slots k_msm_sort keeps for one window.
TMV_HD uint32_t split_max_for(uint32_t m, uint32_t want) {
  const uint32_t most = (m - 1) / 2;
  return want < most ? want : most;
}

}  // namespace tmv
