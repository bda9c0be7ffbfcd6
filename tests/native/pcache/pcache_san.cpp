// Stand-alone sanitizer run of the point cache's host code (pcachecheck.cpp):
// pseudo-random keys and the small-order edge encodings through the checked
// load and a two-bucket table.  Exit status 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int64_t pcachecheck_checked_load(const uint8_t *keys, uint32_t n, uint8_t *decodable);
extern "C" int64_t pcachecheck_table(const uint8_t *keys, uint32_t n, uint32_t slots, uint8_t *hits);

int main() {
  const uint32_t n = 2000;
  std::vector<uint8_t> keys(32 * n), flag(n);
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (auto &b : keys) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    b = (uint8_t)(s >> 32);
  }
  // edge encodings: y = 0, 1, p - 1, p, p + 1 with both sign bits
  const uint8_t lows[5] = {0x00, 0x01, 0xec, 0xed, 0xee};
  for (int e = 0; e < 10; e++) {
    uint8_t *k = &keys[32 * e];
    const bool big = e >= 4;
    for (int i = 0; i < 32; i++) k[i] = big ? 0xff : 0x00;
    k[0] = lows[e / 2];
    k[31] = (uint8_t)((big ? 0x7f : 0x00) | ((e & 1) ? 0x80 : 0x00));
  }
  const int64_t good = pcachecheck_checked_load(keys.data(), n, flag.data());
  if (good <= 0) { std::printf("checked load: %lld\n", (long long)good); return 1; }
  for (uint32_t slots : {4u, 4096u}) {
    const int64_t served = pcachecheck_table(keys.data(), n, slots, flag.data());
    if (served <= 0) { std::printf("table %u: %lld\n", slots, (long long)served); return 1; }
  }
  std::printf("ok %lld decodable of %u\n", (long long)good, n);
  return 0;
}
