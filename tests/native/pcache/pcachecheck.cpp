// Host build of the point cache's hash and checked load (point_cache.h) with
// limb-bound assertions (TMV_BOUNDS_CHECK), against ge_decode_zip215.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../../tendermint_amd/csrc/point_cache.h"

using namespace tmv;

static void words_of(uint32_t w[8], const uint8_t *b) {
  for (int i = 0; i < 8; i++)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}

extern "C" void pcachecheck_hash(const uint8_t *keys, uint32_t n, uint32_t *out) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t w[8];
    words_of(w, keys + 32 * i);
    out[i] = pc_hash(w);
  }
}

extern "C" uint32_t pcachecheck_round_slots(uint64_t slots) { return pc_round_slots(slots); }

// first word (in 32-bit words) of key i's slot in a table of `slots` slots
extern "C" uint64_t pcachecheck_slot_word(const uint8_t key[32], uint32_t slots) {
  uint32_t w[8];
  words_of(w, key);
  return 4 * (uint64_t)pc_slot_quad(pc_hash(w), slots / kPcWays - 1);
}

static bool same_point(const ge_p3 &a, const ge_p3 &b) {
  return fe_eq(a.X, b.X) && fe_eq(a.Y, b.Y) && fe_eq(a.Z, b.Z) && fe_eq(a.T, b.T);
}

// For every key: the checked load accepts exactly the x ge_decode_zip215
// chose (and returns the same point, every coordinate at level 1), and
// rejects -x, x + 1, 0, another key's x and random words; for an undecodable
// key it rejects everything.  Returns the number of decodable keys, or
// -(1000 * step + ...) at the first violation.  decodable[i] is set per key.
extern "C" int64_t pcachecheck_checked_load(const uint8_t *keys, uint32_t n, uint8_t *decodable) {
  int64_t good = 0;
  uint32_t prev_x[8] = {0x12345678u, 1, 2, 3, 4, 5, 6, 7};
  for (uint32_t i = 0; i < n; i++) {
    uint32_t key[8], xw[8], t[8];
    words_of(key, keys + 32 * i);
    ge_p3 P, Q;
    const bool ok = ge_decode_zip215(P, key);
    decodable[i] = ok ? 1 : 0;
    if (!ok) {
      const uint32_t zero[8] = {0}, one[8] = {1};
      if (pc_checked_point(Q, key, zero) || pc_checked_point(Q, key, one) || pc_checked_point(Q, key, prev_x))
        return -(int64_t)(1000 + i);
      continue;
    }
    good++;
    fe_to_words(xw, P.X);
    if (!pc_checked_point(Q, key, xw)) return -(int64_t)(2000000 + i);
    if (!same_point(P, Q)) return -(int64_t)(3000000 + i);
    for (int c = 0; c < 10; c++) {  // level 1, with no slack beyond the macro's
      const int64_t b = (int64_t)1 << ((c & 1) ? 24 : 25);
      const fe *f[3] = {&Q.X, &Q.Y, &Q.T};
      for (int k = 0; k < 3; k++)
        if (f[k]->v[c] > b + (1 << 20) || f[k]->v[c] < -b - (1 << 20)) return -(int64_t)(4000000 + i);
    }
    const bool x_zero = fe_is_zero(P.X);
    fe nx;
    fe_neg(nx, P.X);
    fe_to_words(t, nx);
    if (pc_checked_point(Q, key, t) != x_zero) return -(int64_t)(5000000 + i);  // -x: only when x == 0
    std::memcpy(t, xw, sizeof(t));
    t[0] ^= 1;
    if (pc_checked_point(Q, key, t)) return -(int64_t)(6000000 + i);
    const uint32_t zero[8] = {0};
    if (pc_checked_point(Q, key, zero) != x_zero) return -(int64_t)(7000000 + i);
    if (std::memcmp(prev_x, xw, sizeof(xw)) != 0 && !x_zero) {
      fe px;
      fe_from_words(px, prev_x);
      if (!fe_eq(px, P.X) && pc_checked_point(Q, key, prev_x)) return -(int64_t)(8000000 + i);
    }
    std::memcpy(prev_x, xw, sizeof(xw));
  }
  return good;
}

// The table on the host: insert every decodable key, then probe every key.
// hits[i]: the probe served key i.  A served point equals the decode's.
extern "C" int64_t pcachecheck_table(const uint8_t *keys, uint32_t n, uint32_t slots, uint8_t *hits) {
  std::vector<pc_quad> table((size_t)slots * 4, pc_quad{{0, 0, 0, 0}});
  const uint32_t mask = slots / kPcWays - 1;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t key[8];
    words_of(key, keys + 32 * i);
    ge_p3 P;
    if (ge_decode_zip215(P, key)) pc_insert(table.data(), mask, key, P.X);
  }
  int64_t served = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t key[8];
    words_of(key, keys + 32 * i);
    ge_p3 P, Q;
    hits[i] = pc_probe(Q, table.data(), mask, key) ? 1 : 0;
    if (hits[i]) {
      served++;
      if (!ge_decode_zip215(P, key) || !same_point(P, Q)) return -(int64_t)(1 + i);
    }
  }
  return served;
}
