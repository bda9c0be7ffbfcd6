// Host build of the comb-table code of tendermint_amd/csrc/secp256k1.h (the
// cached-key path) with limb-bound assertions, behind a small C interface for
// tests/test_secp256k1_comb.py.  Combs are kept per key for the library's
// lifetime, as the device keeps them per slot.
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "../../../tendermint_amd/csrc/secp256k1.h"

using namespace tmv::secp;

namespace {

struct KeyComb {
  bool ok;
  std::vector<uint32_t> w;
};
std::map<std::array<uint8_t, 33>, KeyComb> g_combs;

const KeyComb &comb_of(const uint8_t *pk33) {
  std::array<uint8_t, 33> k;
  std::memcpy(k.data(), pk33, 33);
  auto it = g_combs.find(k);
  if (it == g_combs.end()) {
    KeyComb c;
    c.w.resize(kCombWords);
    c.ok = build_key_comb(c.w.data(), pk33);
    it = g_combs.emplace(k, std::move(c)).first;
  }
  return it->second;
}

}  // namespace

extern "C" {

int secpcomb_words(void) { return kCombWords; }

// The whole comb of a key (one inversion per key); 1 when the key parses.
int secpcomb_key(const uint8_t *pk33, uint32_t *out) {
  const KeyComb &c = comb_of(pk33);
  std::memcpy(out, c.w.data(), kCombBytes);
  return c.ok ? 1 : 0;
}

void secpcomb_g(uint32_t *out) { std::memcpy(out, g_comb_host(), kCombBytes); }

// Window j of a key's comb as a lane of k_secp_key_table computes it: 252
// doubling steps of which the first 4 j take effect, the 15 multiples, one
// inversion for the window.  out: 15 entries of 16 words.
int secpcomb_window(const uint8_t *pk33, int j, uint32_t *out) {
  uint32_t xw[8];
  words_from_be32(xw, pk33 + 1);
  ge q;
  const bool ok = ge_decompress(q, pk33[0], xw);
  gej base;
  gej_set_ge(base, q);
  for (int i = 0; i < 4 * (kCombWindows - 1); i++) {
    gej d;
    gej_double(d, base);
    gej_cmov(base, d, i < 4 * j);
  }
  gej pts[kWindowEntries];
  fe pre[kWindowEntries];
  comb_window_multiples(pts, base);
  comb_store_affine(out, pts, pre, kWindowEntries);
  return ok ? 1 : 0;
}

// The cached path's verdict for one signature over the digest z32.
int secpcomb_verify(const uint8_t *pk33, const uint8_t *z32, const uint8_t *sig64) {
  const KeyComb &c = comb_of(pk33);
  return secp256k1_verify_comb(c.ok, c.w.data(), z32, sig64) ? 1 : 0;
}

// The uncached host verdict (secp256k1_verify), for comparison.
int secpcomb_verify_plain(const uint8_t *pk33, const uint8_t *z32, const uint8_t *sig64) {
  return secp256k1_verify(pk33, z32, sig64) ? 1 : 0;
}
}
