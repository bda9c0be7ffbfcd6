// C entry points over csrc/host/key_order.h for tests/test_key_order.py.  The
// arrays the header writes sit between guard words here, laid out as the
// runtime lays them out (the run arrays through KeyRunRegion).
#include <cstring>
#include <vector>

#include "host/key_order.h"

namespace {
constexpr uint32_t kGuard = 0x9e3779b9u, kGuardWords = 8, kUnwritten = 0xeeeeeeeeu;

// `words` words between two runs of guard words.
struct Guarded {
  std::vector<uint32_t> buf;
  explicit Guarded(size_t words) : buf(words + 2 * kGuardWords, kUnwritten) {
    for (uint32_t i = 0; i < kGuardWords; i++) buf[i] = buf[buf.size() - 1 - i] = kGuard;
  }
  uint32_t *data() { return buf.data() + kGuardWords; }
  bool intact() const {
    for (uint32_t i = 0; i < kGuardWords; i++)
      if (buf[i] != kGuard || buf[buf.size() - 1 - i] != kGuard) return false;
    return true;
  }
};
}  // namespace

extern "C" {

uint32_t ko_sort_chunks() { return tmh::kKeySortChunks; }

// hist_out: kKeySortChunks * kc words.  Returns distinct, or -1 for a write outside them.
int64_t ko_histogram(const uint32_t *slots, uint32_t n, uint32_t kc, uint32_t *hist_out) {
  const size_t words = (size_t)tmh::kKeySortChunks * kc;
  Guarded hist(words);
  const uint32_t distinct = tmh::key_histogram(slots, n, kc, hist.data());
  std::memcpy(hist_out, hist.data(), 4 * words);
  return hist.intact() ? (int64_t)distinct : -1;
}

int ko_merge_worth(uint32_t distinct, uint32_t groups, uint32_t n) { return tmh::key_merge_worth(distinct, groups, n); }

// run_cap, slot_at, group_run0_at, words, bytes
void ko_region(uint32_t distinct, uint32_t G, uint64_t *out5) {
  const tmh::KeyRunRegion R(distinct, G);
  const uint64_t v[5] = {R.run_cap, R.slot_at, R.group_run0_at, R.words, R.bytes()};
  for (int k = 0; k < 5; k++) out5[k] = v[k];
}

// Both steps.  order_out: n; lo_out: run_cap + 1; slot_out: run_cap; group_run0_out: G + 1, where
// run_cap = distinct + G; words the header did not write come back as 0xeeeeeeee.  Returns n_runs, or -1 for a
// write outside the arrays.
int64_t ko_order_runs(const uint32_t *slots, uint32_t n, uint32_t kc, uint32_t m_log2, uint32_t G,
                      uint32_t *distinct_out, uint32_t *order_out, uint32_t *lo_out, uint32_t *slot_out,
                      uint32_t *group_run0_out) {
  Guarded hist((size_t)tmh::kKeySortChunks * kc);
  const uint32_t distinct = *distinct_out = tmh::key_histogram(slots, n, kc, hist.data());
  const tmh::KeyRunRegion R(distinct, G);
  Guarded order(n), runs(R.words);
  uint32_t *r = runs.data();
  const uint32_t n_runs =
      tmh::key_order_runs(hist.data(), slots, n, kc, m_log2, G, order.data(), r, r + R.slot_at, r + R.group_run0_at);
  std::memcpy(order_out, order.data(), 4ull * n);
  std::memcpy(lo_out, r, 4 * (R.run_cap + 1));
  std::memcpy(slot_out, r + R.slot_at, 4 * R.run_cap);
  std::memcpy(group_run0_out, r + R.group_run0_at, 4ull * (G + 1));
  return hist.intact() && order.intact() && runs.intact() ? (int64_t)n_runs : -1;
}

}  // extern "C"
