// csrc/host/key_order.h under ASan + UBSan as a stand-alone program: the
// histogram, the order and the runs over the shapes at which their bookkeeping
// can go wrong and over random ones, every array a heap buffer of exactly the
// size the header promises to stay inside (an overrun is an ASan report),
// against a stable sort and a scan of the sorted entries.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <numeric>
#include <vector>

#include "host/key_order.h"

static int g_wrong = 0, g_cases = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok && g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

static void check(const std::vector<uint32_t> &slots, uint32_t kc, uint32_t m_log2) {
  g_cases++;
  const uint32_t n = (uint32_t)slots.size(), m = 1u << m_log2, G = (n + m - 1) >> m_log2;
  // the restatement: stable sort, then a run starts where the key changes or a group does
  std::vector<uint32_t> ref(n);
  std::iota(ref.begin(), ref.end(), 0u);
  std::stable_sort(ref.begin(), ref.end(), [&](uint32_t a, uint32_t b) { return slots[a] < slots[b]; });
  std::vector<uint32_t> rlo, rslot, rg0(G + 1, 0);
  for (uint32_t e = 0; e < n; e++)
    if (e == 0 || e % m == 0 || slots[ref[e]] != slots[ref[e - 1]]) {
      rlo.push_back(e);
      rslot.push_back(slots[ref[e]]);
    }
  for (uint32_t g = 0; g <= G; g++)
    rg0[g] = (uint32_t)(std::lower_bound(rlo.begin(), rlo.end(), std::min<uint64_t>((uint64_t)g * m, n)) - rlo.begin());
  std::vector<uint32_t> sorted_keys(slots);
  std::sort(sorted_keys.begin(), sorted_keys.end());
  const uint32_t ref_distinct = (uint32_t)(std::unique(sorted_keys.begin(), sorted_keys.end()) - sorted_keys.begin());

  std::unique_ptr<uint32_t[]> hist(new uint32_t[(size_t)tmh::kKeySortChunks * kc]);
  const uint32_t distinct = tmh::key_histogram(slots.data(), n, kc, hist.get());
  expect(distinct == ref_distinct, "distinct", distinct, ref_distinct);
  uint64_t counted = 0;
  for (size_t i = 0; i < (size_t)tmh::kKeySortChunks * kc; i++) counted += hist[i];
  expect(counted == n, "histogram total", counted, n);
  const tmh::KeyRunRegion R(distinct, G);
  expect(R.bytes() == 4 * (2 * R.run_cap + 1 + G + 1) && R.slot_at == R.run_cap + 1 &&
             R.group_run0_at == R.slot_at + R.run_cap && R.words == R.group_run0_at + G + 1,
         "region", R.words, R.run_cap);
  std::unique_ptr<uint32_t[]> order(new uint32_t[n]), lo(new uint32_t[R.run_cap + 1]), slot(new uint32_t[R.run_cap]),
      g0(new uint32_t[G + 1]);
  const uint32_t n_runs =
      tmh::key_order_runs(hist.get(), slots.data(), n, kc, m_log2, G, order.get(), lo.get(), slot.get(), g0.get());
  expect(n_runs == rlo.size() && n_runs <= R.run_cap, "n_runs", n_runs, rlo.size());
  if (n_runs != rlo.size()) return;
  expect(std::equal(ref.begin(), ref.end(), order.get()), "order", n, kc);
  expect(std::equal(rlo.begin(), rlo.end(), lo.get()) && lo[n_runs] == n, "lo", n, n_runs);
  expect(std::equal(rslot.begin(), rslot.end(), slot.get()), "slot", n, n_runs);
  expect(std::equal(rg0.begin(), rg0.end(), g0.get()) && g0[G] == n_runs, "group_run0", n, G);
  for (uint32_t r = 0; r < n_runs; r++) {
    expect(lo[r] < lo[r + 1], "lo strictly increasing", r, lo[r]);
    expect(lo[r] >> m_log2 == (lo[r + 1] - 1) >> m_log2, "run inside one group", r, lo[r]);
    for (uint32_t e = lo[r]; e < lo[r + 1]; e++) expect(slots[order[e]] == slot[r], "run of one key", r, e);
  }
}

int main() {
  uint64_t x = 88172645463325252ull;
  auto rnd = [&x](uint32_t mod) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return (uint32_t)(x % mod);
  };
  for (uint32_t m_log2 : {6u, 7u}) {
    const uint32_t m = 1u << m_log2;
    for (uint32_t n : {1u, 2u, 15u, 16u, 17u, m - 1, m, m + 1, 2 * m, 3 * m + 5}) {
      check(std::vector<uint32_t>(n, 0), 1, m_log2);             // kc = 1
      check(std::vector<uint32_t>(n, 3), 5, m_log2);             // one key on every entry: a run per group
      std::vector<uint32_t> all(n), gaps(n), inter(n), rand_slots(n);
      for (uint32_t i = 0; i < n; i++) {
        all[i] = n - 1 - i;                                      // all keys distinct, in reverse
        gaps[i] = 3 + 7 * (i % 5);                               // slot ids with gaps
        inter[i] = i % 3;                                        // three keys interleaved
        rand_slots[i] = rnd(11);
      }
      check(all, n, m_log2);
      check(all, n + 9, m_log2);
      check(gaps, 40, m_log2);
      check(inter, 3, m_log2);
      check(rand_slots, 11, m_log2);
    }
    // a key whose segment ends exactly on a group edge and one that starts on it; then a long key
    // over three groups, so that groups hold no run start but the cut
    std::vector<uint32_t> edge;
    edge.insert(edge.end(), m - 10, 1);
    edge.insert(edge.end(), 10, 4);
    edge.insert(edge.end(), 3 * m + 1, 6);
    edge.insert(edge.end(), 7, 9);
    check(edge, 10, m_log2);
    std::reverse(edge.begin(), edge.end());
    check(edge, 10, m_log2);
    for (int t = 0; t < 40; t++) {
      const uint32_t n = 1 + rnd(5 * m), kc = 1 + rnd(300), keys = 1 + rnd(kc);
      std::vector<uint32_t> s(n);
      for (uint32_t &v : s) v = rnd(keys);
      check(s, kc, m_log2);
    }
  }
  // the merge rule at its boundary
  expect(tmh::key_merge_worth(10, 22, 64), "worth it at n / 2", 32, 64);
  expect(tmh::key_merge_worth(10, 22, 65), "n / 2 rounds down", 32, 65);
  expect(!tmh::key_merge_worth(11, 22, 65), "one above", 33, 65);
  expect(!tmh::key_merge_worth(0xffffffffu, 1, 0xffffffffu), "sum does not wrap", 0, 0);
  std::printf("%d cases, %d wrong\n", g_cases, g_wrong);
  return g_wrong ? 1 : 0;
}
