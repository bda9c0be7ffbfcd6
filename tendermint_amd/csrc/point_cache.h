// Per-device table of decoded ed25519 public keys (the point cache).
//
// A validator set signs every block, so the batches a node drains carry the
// same public keys over and over; the table lets the prep skip the square
// root (255 squarings) for a key the device has decoded before.
//
// Layout: buckets of kPcWays entries of 64 bytes -- the raw 32-byte encoding
// (sign bit included), then the canonical x chosen for it -- so a bucket is
// one 128-byte line.  The bucket and the way both come from pc_hash of the
// key: a key has exactly one slot, a probe reads that slot alone, an insert
// is a plain overwrite, there is no LRU and no lock.
//
// A HIT IS CHECKED, NEVER TRUSTED.  Streams share the table without any
// synchronisation, so a probe may read a torn entry (a racing writer), a
// stale one, or garbage.  pc_checked_point therefore takes y from the
// encoding exactly as ge_decode_zip215 does and accepts the entry's x only if
//   x^2 (d y^2 + 1) == y^2 - 1   and   (parity(x) == bit 255  or  x == 0),
// which names the one x ge_decode_zip215 returns for that encoding (the curve
// equation has the roots +-x, the sign bit picks one; d y^2 + 1 is never 0;
// an undecodable encoding has no root, so nothing passes for it).  Anything
// else is a miss and takes the ordinary decode.  The validity vector is thus
// a function of the inputs alone, for any table contents and any interleaving
// of launches; keys are attacker-chosen, and a thrashed table only costs the
// old decode.
//
// Compiled for the device (verify_kernels.hip) and, unchanged, for the host
// (tests/native/pcache/pcachecheck.cpp, with limb-bound assertions).
#pragma once
#include "curve25519.h"

namespace tmv {

constexpr uint32_t kPcWays = 2;          // entries per bucket (one 128-byte line)
constexpr uint32_t kPcEntryWords = 16;   // key (8 words), x (8 words)
constexpr uint32_t kPcBucketWords = kPcWays * kPcEntryWords;
constexpr uint32_t kPcMaxSlots = 1u << 24;  // 1 GiB

struct alignas(16) pc_quad { uint32_t v[4]; };

// View of the table a launch carries (Ed25519Work::pc).  table == nullptr:
// off.  counters: [0] hits, [1] misses.
struct PointCache {
  pc_quad *table;
  unsigned long long *counters;
  uint32_t bucket_mask;  // buckets - 1 (a power of two)
  uint32_t min_n;        // launches below this many entries decode as before
};

// Slots the table really has for a requested capacity: the largest power of
// two <= slots, at least one bucket, at most kPcMaxSlots; 0 stays 0 (off).
inline uint32_t pc_round_slots(uint64_t slots) {
  if (slots == 0) return 0;
  if (slots < kPcWays) return kPcWays;
  uint32_t s = kPcWays;
  while (2ull * s <= slots && s < kPcMaxSlots) s *= 2;
  return s;
}

TMV_HD uint32_t pc_mix(uint32_t h) {  // murmur3's finalizer
  h ^= h >> 16; h *= 0x85ebca6bu;
  h ^= h >> 13; h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// Three words of the key, the one holding the sign bit among them (two keys
// that differ only in bit 255 do not share a slot).
TMV_HD uint32_t pc_hash(const uint32_t w[8]) {
  return pc_mix(w[0] ^ pc_mix(w[3] ^ pc_mix(w[7] ^ 0x9e3779b9u)));
}
// First quad of the key's slot.
TMV_HD size_t pc_slot_quad(uint32_t h, uint32_t bucket_mask) {
  return ((size_t)(h & bucket_mask) * kPcWays + (h >> 31)) * (kPcEntryWords / 4);
}

// Values read from the shared table go through this before use, so the
// compiler can never read the location again after the check.
TMV_HD void pc_launder(uint32_t &x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#else
  (void)x;
#endif
}

// The point of encoding `key` from a candidate x (canonical words, as
// fe_to_words writes them): true and P = (x, y, 1, x y) with the limb bounds
// of a freshly decoded point (every coordinate level 1), or false.
TMV_HD bool pc_checked_point(ge_p3 &P, const uint32_t key[8], const uint32_t xw[8]) {
  fe x, yy, xx, u, v, one, chk;
  fe_from_words(P.Y, key);
  fe_carry(P.Y, P.Y);                  // as ge_decode_zip215: level 1
  fe_from_words(x, xw);
  fe_carry(x, x);                      // level 1
  fe_one(one);
  fe_sq(yy, P.Y);
  fe_mul(v, yy, consts::d());
  fe_sub(u, yy, one);                  // u = y^2 - 1      (2)
  fe_add(v, v, one);                   // v = d y^2 + 1    (2)
  fe_sq(xx, x);
  fe_mul(xx, xx, v);
  fe_sub(chk, xx, u);                  // 3
  if (!fe_is_zero(chk)) return false;
  const bool sign = (key[7] >> 31) & 1;
  if (fe_is_negative(x) != sign && !fe_is_zero(x)) return false;
  P.X = x;
  fe_one(P.Z);
  fe_mul(P.T, P.X, P.Y);
  TMV_ASSERT_LEVEL(P.X, 1);
  TMV_ASSERT_LEVEL(P.Y, 1);
  TMV_ASSERT_LEVEL(P.T, 1);
  return true;
}

// Probe: only the key's own way of its bucket can hold it (an all-zero key
// would otherwise match an empty neighbour), so the probe reads that slot --
// half a line -- and hands its x to the checked load when the 32 key bytes
// match.
TMV_HD bool pc_probe(ge_p3 &P, const pc_quad *table, uint32_t bucket_mask, const uint32_t key[8]) {
  const pc_quad *s = table + pc_slot_quad(pc_hash(key), bucket_mask);
  const pc_quad k0 = s[0], k1 = s[1], x0 = s[2], x1 = s[3];
  uint32_t diff = 0, xw[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    diff |= (k0.v[i] ^ key[i]) | (k1.v[i] ^ key[4 + i]);
    xw[i] = x0.v[i];
    xw[4 + i] = x1.v[i];
    pc_launder(xw[i]);
    pc_launder(xw[4 + i]);
  }
  if (diff != 0) return false;
  return pc_checked_point(P, key, xw);
}

// Insert a decoded key (X level <= 3): overwrites the key's slot.
TMV_HD void pc_insert(pc_quad *table, uint32_t bucket_mask, const uint32_t key[8], const fe &X) {
  uint32_t xw[8];
  fe_to_words(xw, X);
  pc_quad *s = table + pc_slot_quad(pc_hash(key), bucket_mask);
  s[0] = pc_quad{{key[0], key[1], key[2], key[3]}};
  s[1] = pc_quad{{key[4], key[5], key[6], key[7]}};
  s[2] = pc_quad{{xw[0], xw[1], xw[2], xw[3]}};
  s[3] = pc_quad{{xw[4], xw[5], xw[6], xw[7]}};
}

}  // namespace tmv
