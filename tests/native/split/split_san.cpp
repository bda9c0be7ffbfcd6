// ASan + UBSan run of split.h's digit map through splitcheck.cpp (CPU only):
// for every window size and group size, edge and random scalars are recoded,
// relabelled and summed back with a small multi-word accumulator.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

extern "C" int splitcheck_params(uint32_t c, uint32_t m_log2, uint32_t *out);
extern "C" int splitcheck_entries(const uint32_t *s, uint32_t c, uint32_t m_log2, int32_t *lo, int32_t *hi,
                                  uint32_t *unsplit, uint32_t *top_hi);

namespace {
// x = x * 2^c + d over 10 words (two's complement; the totals stay far below 2^319)
void step(uint32_t x[10], uint32_t c, int32_t d) {
  for (int k = 9; k > 0; k--) x[k] = (x[k] << c) | (x[k - 1] >> (32 - c));
  x[0] <<= c;
  const uint32_t ext = d < 0 ? 0xffffffffu : 0u;  // d sign-extended
  uint64_t carry = 0;
  for (int k = 0; k < 10; k++) {
    const uint64_t t = (uint64_t)x[k] + (k == 0 ? (uint32_t)d : ext) + carry;
    x[k] = (uint32_t)t;
    carry = t >> 32;
  }
}
}  // namespace

int main() {
  // l - 1
  const uint32_t lm1[8] = {0x5cf5d3ecu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
  std::mt19937 rng(5);
  long checked = 0;
  for (uint32_t c = 4; c <= 9; c++)
    for (uint32_t m_log2 = 5; m_log2 <= 10; m_log2++) {
      uint32_t prm[9];
      if (splitcheck_params(c, m_log2, prm)) return 1;
      const uint32_t W = prm[0], Ws = prm[3];
      std::vector<std::vector<uint32_t>> cases;
      cases.push_back(std::vector<uint32_t>(8, 0));
      cases.push_back({1, 0, 0, 0, 0, 0, 0, 0});
      cases.push_back(std::vector<uint32_t>(lm1, lm1 + 8));
      for (int delta = -1; delta <= 0; delta++) {  // 2^(c Ws) - 1, 2^(c Ws)
        std::vector<uint32_t> v(8, 0);
        const uint32_t bit = c * Ws;
        if (delta == 0) v[bit >> 5] = 1u << (bit & 31);
        else for (uint32_t b = 0; b < bit; b++) v[b >> 5] |= 1u << (b & 31);
        cases.push_back(v);
      }
      for (int t = 0; t < 200; t++) {
        std::vector<uint32_t> v(8);
        for (auto &x : v) x = rng();
        v[7] &= 0x0fffffffu;  // below 2^252 < l
        cases.push_back(v);
      }
      std::vector<int32_t> lo(W), hi(W);
      for (const auto &v : cases) {
        uint32_t unsplit = 0, top = 0;
        const int n = splitcheck_entries(v.data(), c, m_log2, lo.data(), hi.data(), &unsplit, &top);
        if (n < 0 || (uint32_t)n != unsplit || top > Ws) { fprintf(stderr, "entries c=%u\n", c); return 1; }
        uint32_t x[10] = {0};
        for (int w = (int)Ws - 1; w >= 0; w--) step(x, c, hi[w]);  // the high half, then the low one below it
        for (int w = (int)Ws - 1; w >= 0; w--) step(x, c, lo[w]);
        for (uint32_t w = Ws; w < W; w++)
          if (lo[w] || hi[w]) { fprintf(stderr, "window past Ws c=%u\n", c); return 1; }
        uint32_t want[10] = {0};
        memcpy(want, v.data(), 32);
        if (memcmp(x, want, sizeof(x))) { fprintf(stderr, "sum differs c=%u m_log2=%u\n", c, m_log2); return 1; }
        checked++;
      }
    }
  printf("split_san ok: %ld scalars\n", checked);
  return 0;
}
