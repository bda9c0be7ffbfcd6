// Host entry points over tendermint_amd/csrc/split.h (with msm.h's
// parameters and signed-digit recoding) for tests/test_scalar_split.py and
// split_san.cpp.
#include <cstddef>
#include <cstdint>
#include "../../../tendermint_amd/csrc/msm.h"

// out[0..8] = W, WR, WL, Ws, Wa, Wl, cap, H, m of a group of 2^m_log2 with c-bit windows.
extern "C" int splitcheck_params(uint32_t c, uint32_t m_log2, uint32_t *out) {
  if (c < 4 || c > 9 || m_log2 < 5 || m_log2 > 10) return -1;
  const tmv::MsmParams p = tmv::MsmParams::make(1u << m_log2, m_log2, c);
  out[0] = p.W; out[1] = p.WR; out[2] = p.WL(); out[3] = p.Ws; out[4] = p.Wa; out[5] = p.Wl;
  out[6] = p.cap; out[7] = p.H; out[8] = p.m();
  return 0;
}

extern "C" uint32_t splitcheck_split_max(uint32_t m, uint32_t want) { return tmv::split_max_for(m, want); }

// The entries of scalar s (8 words, < 2^254) in a split group: lo[w] / hi[w]
// = the digit whose entry is (window w, P) / (window w, P_hi), 0 = none, for
// w < W.  Returns the number of entries, -1 for bad arguments, -2 if two
// digits land on one (window, point).  *unsplit = the unsplit recoding's
// entry count, *top_hi = 1 + the highest window holding a high entry.
extern "C" int splitcheck_entries(const uint32_t *s, uint32_t c, uint32_t m_log2, int32_t *lo, int32_t *hi,
                                  uint32_t *unsplit, uint32_t *top_hi) {
  if (c < 4 || c > 9 || m_log2 < 5 || m_log2 > 10) return -1;
  const tmv::MsmParams p = tmv::MsmParams::make(1u << m_log2, m_log2, c);
  for (uint32_t w = 0; w < p.W; w++) lo[w] = hi[w] = 0;
  int carry = 0, n = 0;
  *unsplit = 0;
  *top_hi = 0;
  for (uint32_t w = 0; w < p.W; w++) {
    const int d = tmv::sc_window_digit(s, 8, w, c, w + 1 == p.W, carry);
    if (d == 0) continue;
    const tmv::SplitSlot plain = tmv::split_slot(w, p.Ws, false);
    if (plain.hi || plain.window != w) return -2;
    (*unsplit)++;
    const tmv::SplitSlot ss = tmv::split_slot(w, p.Ws, true);
    if (ss.window >= p.W) return -2;
    int32_t *cell = (ss.hi ? hi : lo) + ss.window;
    if (*cell) return -2;
    *cell = d;
    if (ss.hi && ss.window + 1 > *top_hi) *top_hi = ss.window + 1;
    n++;
  }
  return n;
}
