// Stand-alone sanitizer run of the column order's slot function
// (colordercheck.cpp): ragged launches with empty batches at every batch
// count around the tile height, equal-size launches, and T = 0.  Exit status
// 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int64_t colordercheck_permutation(const uint32_t *counts, uint32_t K, uint32_t T, uint32_t *idx_out);
extern "C" int64_t colordercheck_slot(const uint32_t *counts, uint32_t K, uint32_t T, uint32_t j, uint32_t i);

int main() {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&](uint32_t mod) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (uint32_t)((s >> 33) % mod);
  };
  const uint32_t Ks[] = {1, 2, 63, 64, 65, 256};
  const uint32_t Ts[] = {0, 1, 3, 64, 256};
  for (uint32_t K : Ks)
    for (uint32_t T : Ts)
      for (int round = 0; round < 3; round++) {
        std::vector<uint32_t> counts(K);
        uint32_t N = 0;
        for (auto &c : counts) {
          c = round == 0 ? 37 : (rnd(4) == 0 ? 0 : rnd(90));
          N += c;
        }
        std::vector<uint32_t> idx(N + 1, 0);
        const int64_t bad = colordercheck_permutation(counts.data(), K, T, idx.data());
        if (bad != 0) { std::printf("K=%u T=%u round %d: %lld bad slots\n", K, T, round, (long long)bad); return 1; }
        for (uint32_t e = 0; e < N; e++) {
          if (idx[e] == 0xffffffffu) { std::printf("K=%u T=%u: slot %u empty\n", K, T, e); return 1; }
          if ((T == 0 || K == 1) && idx[e] != e) { std::printf("K=%u T=%u: not the identity\n", K, T); return 1; }
        }
        if (round == 0 && T > 0 && K > 1) {  // equal sizes: slots [c T', (c+1) T') of a tile are column c
          const uint32_t j = K - 1, t0 = j / T * T, rows = K - t0 < T ? K - t0 : T;
          const int64_t got = colordercheck_slot(counts.data(), K, T, j, 5);
          const int64_t want = (int64_t)t0 * 37 + 5 * rows + (j - t0);
          if (got != want) { std::printf("K=%u T=%u: slot %lld, expected %lld\n", K, T, (long long)got, (long long)want); return 1; }
        }
      }
  std::printf("ok\n");
  return 0;
}
