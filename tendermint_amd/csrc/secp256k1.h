// GF(2^256 - 2^32 - 977) field, secp256k1 group, scalars mod n and ECDSA
// verification for the MI355X kernels.  Compiled for gfx950 (device) and,
// unchanged, for the host: the runtime builds the G table with it, the host
// layer verifies with it where no device entry is linked, and the CPU test
// (tests/native/secp/secpcheck.cpp) runs it with limb-bound assertions.
//
// Replaces crypto/secp256k1/secp256k1.go:206-226 (PubKey.VerifySignature over
// btcec v0.22.1 ParsePubKey and Go's ecdsa.Verify): compressed 33-byte keys
// only (the one size crypto/encoding/codec.go:49-78 admits), lower-S
// signatures only, every failure a plain `false`.
//
// Field representation: ten unsigned 26-bit limbs (the top limb 22 bits).
// One field multiply = 100 32x32->64 multiply-adds (v_mad_u64_u32 columns),
// 19 columns folded with 2^260 == 2^36 + 15632 (16 * (2^32 + 977)).
//
// Limb-magnitude discipline: "magnitude m" means limb i <= 2m(2^26 - 1)
// (limb 9: 2m(2^22 - 1)).  Every mul/sq output has magnitude 1; sums add
// magnitudes; fe_neg(a, m) gives m + 1.  Multiply inputs must have magnitude
// <= 8 (limbs < 2^30: ten products < 2^63.4 per 64-bit column).  Each formula
// is annotated with the magnitudes of its intermediates; TMV_BOUNDS_CHECK
// (host only) asserts them.
#pragma once
#include <stdint.h>
#include "curve25519.h"  // TMV_HD
#include "sha256_dev.h"

#ifdef TMV_BOUNDS_CHECK
#define SECP_ASSERT_MAG(f, m)                                                        \
  do {                                                                               \
    for (int _i = 0; _i < 10; _i++)                                                  \
      if ((uint64_t)(f).n[_i] > 2ull * (m) * (_i == 9 ? 0x3FFFFFull : 0x3FFFFFFull)) \
        assert(!"secp256k1 field limb exceeds its magnitude bound");                 \
  } while (0)
#else
#define SECP_ASSERT_MAG(f, m) do { } while (0)
#endif

namespace tmv {
namespace secp {

// ------------------------------------------------------------------ field
struct fe { uint32_t n[10]; };

constexpr uint32_t kM26 = 0x3FFFFFFu, kM22 = 0x3FFFFFu;
// p = 2^256 - 2^32 - 977 in 26-bit limbs
TMV_HD uint32_t p_limb(int i) { return i == 0 ? 0x3FFFC2Fu : i == 1 ? 0x3FFFFBFu : i == 9 ? kM22 : kM26; }

TMV_HD void fe_set_int(fe &r, uint32_t a) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = 0;
  r.n[0] = a;
}
TMV_HD void fe_add(fe &r, const fe &a, const fe &b) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = a.n[i] + b.n[i];
}
// r = -a for a of magnitude <= m; r has magnitude m + 1
TMV_HD void fe_neg(fe &r, const fe &a, uint32_t m) {
  SECP_ASSERT_MAG(a, m);
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = 2 * (m + 1) * p_limb(i) - a.n[i];
}
// r = a - b for b of magnitude <= mb; magnitude(a) + mb + 1
TMV_HD void fe_sub(fe &r, const fe &a, const fe &b, uint32_t mb) {
  fe t;
  fe_neg(t, b, mb);
  fe_add(r, a, t);
}
// r = k * a (magnitude k * m)
TMV_HD void fe_mul_int(fe &r, const fe &a, uint32_t k) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = a.n[i] * k;
}
// branch-free conditional move: r = b ? a : r
TMV_HD void fe_cmov(fe &r, const fe &a, bool b) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = b ? a.n[i] : r.n[i];
}

// Column accumulation c + a * b as one v_mad_u64_u32 (curve25519.h mad_acc,
// unsigned): the empty asm keeps each column one multiply-add chain.
TMV_HD uint64_t mad_acc_u(uint32_t a, uint32_t b, uint64_t c) {
  uint64_t r = c + (uint64_t)a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(r));
#endif
  return r;
}

// 19 product columns (c[19] = 0 on entry is not needed: it is written here)
// -> magnitude-1 limbs.
TMV_HD void fe_reduce_columns(fe &r, uint64_t c[20]) {
  constexpr uint32_t R0 = 0x3D10u, R1 = 0x400u;  // 2^260 == R0 + R1 * 2^26
  // carry the columns to 26 bits each; c[19] < 2^38 takes the last carry
  c[19] = 0;
#pragma unroll
  for (int k = 0; k < 19; k++) {
    c[k + 1] += c[k] >> 26;
    c[k] &= kM26;
  }
  // fold positions 10..19 onto 0..10
  uint64_t e[11];
  e[0] = mad_acc_u(R0, (uint32_t)c[10], c[0]);
#pragma unroll
  for (int k = 1; k < 9; k++) e[k] = mad_acc_u(R1, (uint32_t)c[k + 9], mad_acc_u(R0, (uint32_t)c[k + 10], c[k]));
  e[9] = c[9] + (uint64_t)R0 * c[19] + (uint64_t)R1 * (uint32_t)c[18];  // < 2^53
  e[10] = (uint64_t)R1 * c[19];                                          // < 2^48
#pragma unroll
  for (int k = 0; k < 10; k++) {
    e[k + 1] += e[k] >> 26;
    e[k] &= kM26;
  }
  // position 10 (< 2^49) once more; the carries die out within two limbs
  const uint64_t t = e[10];
  e[0] += t * R0;  // < 2^63
  e[1] += t * R1;  // < 2^59
#pragma unroll
  for (int k = 0; k < 9; k++) {
    e[k + 1] += e[k] >> 26;
    e[k] &= kM26;
  }
  // limb 9 holds bits 234..: what is above 2^256 comes back as 2^32 + 977
  const uint32_t x = (uint32_t)(e[9] >> 22);  // < 2^6
  e[9] &= kM22;
  e[0] += (uint64_t)x * 0x3D1u;
  e[1] += (uint64_t)x << 6;
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = (uint32_t)e[i];
  SECP_ASSERT_MAG(r, 1);
}

TMV_HD void fe_mul(fe &r, const fe &a, const fe &b) {
  SECP_ASSERT_MAG(a, 8);
  SECP_ASSERT_MAG(b, 8);
  uint64_t c[20];
#pragma unroll
  for (int i = 0; i < 10; i++) {
#pragma unroll
    for (int j = 0; j < 10; j++) {
      if (i == 0 || j == 9) c[i + j] = (uint64_t)a.n[i] * b.n[j];  // the column's first product
      else c[i + j] = mad_acc_u(a.n[i], b.n[j], c[i + j]);
    }
  }
  fe_reduce_columns(r, c);
}

// r = a^2 (55 products via symmetry)
TMV_HD void fe_sq(fe &r, const fe &a) {
  SECP_ASSERT_MAG(a, 8);
  uint32_t a2[10];
#pragma unroll
  for (int i = 0; i < 10; i++) a2[i] = 2 * a.n[i];  // < 2^31
  uint64_t c[20];
#pragma unroll
  for (int i = 0; i < 10; i++) {
#pragma unroll
    for (int j = i; j < 10; j++) {
      const uint32_t x = i == j ? a.n[i] : a2[i];
      if (i == 0 || j == 9) c[i + j] = (uint64_t)x * a.n[j];
      else c[i + j] = mad_acc_u(x, a.n[j], c[i + j]);
    }
  }
  fe_reduce_columns(r, c);
}

// Full reduction to the canonical representative (limbs 26 bits, value < p).
// Any magnitude whose limbs fit 31 bits.
TMV_HD void fe_normalize(fe &r) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = r.n[i];
  uint32_t x = t[9] >> 22;
  t[9] &= kM22;
  t[0] += x * 0x3D1u;
  t[1] += x << 6;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t[i + 1] += t[i] >> 26;
    t[i] &= kM26;
  }
  // now < 2^256 + 2^230 or so: at most one more p to take off
  bool mid = true;
#pragma unroll
  for (int i = 2; i < 9; i++) mid = mid && t[i] == kM26;
  const bool ge_p = (t[9] >> 22) != 0 ||
                    (t[9] == kM22 && mid && (t[1] > 0x3FFFFBFu || (t[1] == 0x3FFFFBFu && t[0] >= 0x3FFFC2Fu)));
  x = ge_p ? 1u : 0u;
  t[0] += x * 0x3D1u;  // + (2^256 - p), then drop bit 256
  t[1] += x << 6;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t[i + 1] += t[i] >> 26;
    t[i] &= kM26;
  }
  t[9] &= kM22;
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = t[i];
}

// a == 0 mod p, for any magnitude whose limbs fit 31 bits
TMV_HD bool fe_is_zero(const fe &a) {
  fe t = a;
  fe_normalize(t);
  uint32_t z = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) z |= t.n[i];
  return z == 0;
}
// a == b mod p (a: magnitude <= 8, b: magnitude <= mb <= 7)
TMV_HD bool fe_equal(const fe &a, const fe &b, uint32_t mb) {
  fe t;
  fe_sub(t, a, b, mb);
  return fe_is_zero(t);
}
TMV_HD bool fe_is_odd_normalized(const fe &a) { return a.n[0] & 1; }

// 8 little-endian 32-bit words (a value < 2^256) -> limbs (magnitude 1)
TMV_HD void fe_from_words(fe &r, const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 5, s = bit & 31;
    uint64_t v = w[k];
    if (k + 1 < 8) v |= (uint64_t)w[k + 1] << 32;
    r.n[i] = (uint32_t)(v >> s) & kM26;
  }
}
// canonical limbs -> 8 little-endian words
TMV_HD void fe_to_words_normalized(uint32_t w[8], const fe &a) {
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 5, s = bit & 31;
    const uint64_t v = (uint64_t)a.n[i] << s;
    w[k] |= (uint32_t)v;
    if (k + 1 < 8) w[k + 1] |= (uint32_t)(v >> 32);
  }
}
// 32 big-endian bytes -> 8 little-endian words
TMV_HD void words_from_be32(uint32_t w[8], const uint8_t b[32]) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint8_t *q = b + 28 - 4 * k;
    w[k] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}
TMV_HD void words_to_be32(uint8_t b[32], const uint32_t w[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint8_t *q = b + 28 - 4 * k;
    q[0] = (uint8_t)(w[k] >> 24); q[1] = (uint8_t)(w[k] >> 16); q[2] = (uint8_t)(w[k] >> 8); q[3] = (uint8_t)w[k];
  }
}
// a < b over 8 little-endian words, without branches
TMV_HD bool words_less(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t d = (uint64_t)a[k] - b[k] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  return borrow != 0;
}
TMV_HD uint32_t p_word(int k) { return k == 0 ? 0xFFFFFC2Fu : k == 1 ? 0xFFFFFFFEu : 0xFFFFFFFFu; }

// Field element from 8 little-endian words; false when the value is >= p
// (btcec ParsePubKey's x range test)
TMV_HD bool fe_from_words_checked(fe &r, const uint32_t w[8]) {
  uint32_t pw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) pw[k] = p_word(k);
  fe_from_words(r, w);
  return words_less(w, pw);
}
TMV_HD bool fe_from_be32(fe &r, const uint8_t b[32]) {
  uint32_t w[8];
  words_from_be32(w, b);
  return fe_from_words_checked(r, w);
}
TMV_HD void fe_to_be32(uint8_t b[32], const fe &a) {
  fe t = a;
  fe_normalize(t);
  uint32_t w[8];
  fe_to_words_normalized(w, t);
  words_to_be32(b, w);
}

TMV_HD void fe_sqn(fe &r, const fe &a, int n) {
  r = a;
#pragma unroll 1
  for (int i = 0; i < n; i++) fe_sq(r, r);
}

// r = a^((p+1)/4): a square root of a when a is a square (p == 3 mod 4).
// (p+1)/4 = 2^254 - 2^30 - 244 = [223 ones] 0 [22 ones] 0000 11 00 in binary.
// a: magnitude <= 8.
TMV_HD void fe_sqrt_candidate(fe &r, const fe &a) {
  fe x2, x3, x6, x9, x11, x22, x44, x88, x176, x220, x223, t;
  fe_sq(t, a); fe_mul(x2, t, a);
  fe_sq(t, x2); fe_mul(x3, t, a);
  fe_sqn(t, x3, 3); fe_mul(x6, t, x3);
  fe_sqn(t, x6, 3); fe_mul(x9, t, x3);
  fe_sqn(t, x9, 2); fe_mul(x11, t, x2);
  fe_sqn(t, x11, 11); fe_mul(x22, t, x11);
  fe_sqn(t, x22, 22); fe_mul(x44, t, x22);
  fe_sqn(t, x44, 44); fe_mul(x88, t, x44);
  fe_sqn(t, x88, 88); fe_mul(x176, t, x88);
  fe_sqn(t, x176, 44); fe_mul(x220, t, x44);
  fe_sqn(t, x220, 3); fe_mul(x223, t, x3);
  fe_sqn(t, x223, 23); fe_mul(t, t, x22);
  fe_sqn(t, t, 6); fe_mul(t, t, x2);
  fe_sqn(r, t, 2);
}

// r = a^(p-2) (host table build and tests; square-and-multiply over the
// constant exponent: p - 2 has bits 255..33 set, bit 32 clear, low word
// 0xFFFFFC2D)
TMV_HD void fe_inv(fe &r, const fe &a) {
  fe t;
  fe_set_int(t, 1);
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    fe_sq(t, t);
    const bool bit = i >= 33 ? true : i == 32 ? false : ((0xFFFFFC2Du >> i) & 1u) != 0;
    if (bit) fe_mul(t, t, a);
  }
  r = t;
}

// ------------------------------------------------------------------ scalars mod n
struct sc { uint32_t w[8]; };  // little-endian words, value < n unless noted

TMV_HD uint32_t n_word(int k) {
  return k == 0 ? 0xD0364141u : k == 1 ? 0xBFD25E8Cu : k == 2 ? 0xAF48A03Bu : k == 3 ? 0xBAAEDCE6u
       : k == 4 ? 0xFFFFFFFEu : 0xFFFFFFFFu;
}
// 2^256 - n (129 bits)
TMV_HD uint32_t nc_word(int k) {
  return k == 0 ? 0x2FC9BEBFu : k == 1 ? 0x402DA173u : k == 2 ? 0x50B75FC4u : k == 3 ? 0x45512319u : k == 4 ? 1u : 0u;
}

TMV_HD bool sc_is_zero(const sc &a) {
  uint32_t z = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) z |= a.w[k];
  return z == 0;
}
TMV_HD bool sc_below_n(const uint32_t w[8]) {
  uint32_t nw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nw[k] = n_word(k);
  return words_less(w, nw);
}
// a > n >> 1 (the upper-S test of secp256k1.go:220)
TMV_HD bool sc_is_high(const sc &a) {
  uint32_t half[8];
#pragma unroll
  for (int k = 0; k < 8; k++) half[k] = (n_word(k) >> 1) | (k < 7 ? n_word(k + 1) << 31 : 0u);
  return words_less(half, a.w);
}
// r = a - n if a >= n (a: any 256-bit value)
TMV_HD void sc_reduce_once(sc &r, const uint32_t a[8]) {
  uint32_t d[8], borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t t = (uint64_t)a[k] - n_word(k) - borrow;
    d[k] = (uint32_t)t;
    borrow = (uint32_t)(t >> 63);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) r.w[k] = borrow ? a[k] : d[k];
}
// 32 big-endian bytes -> scalar; false when the value is >= n (r then holds value - n)
TMV_HD bool sc_from_be32(sc &r, const uint8_t b[32]) {
  uint32_t w[8];
  words_from_be32(w, b);
  const bool ok = sc_below_n(w);
  sc_reduce_once(r, w);
  return ok;
}

// out[0..NOUT) = in[0..8) + in[8..NIN) * (2^256 - n): one folding step of the
// reduction mod n = 2^256 - c.  The caller picks NOUT so that the value fits.
template <int NIN, int NOUT>
TMV_HD void sc_fold(uint32_t *out, const uint32_t *in) {
  uint32_t acc[NOUT];
#pragma unroll
  for (int k = 0; k < NOUT; k++) acc[k] = k < 8 ? in[k] : 0u;
#pragma unroll
  for (int i = 0; i < NIN - 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = i; k < NOUT; k++) {
      const int j = k - i;
      uint64_t t = (uint64_t)acc[k] + carry;
      if (j < 5) t += (uint64_t)in[8 + i] * nc_word(j);
      acc[k] = (uint32_t)t;
      carry = t >> 32;
    }
  }
#pragma unroll
  for (int k = 0; k < NOUT; k++) out[k] = acc[k];
}

// r = a * b mod n
TMV_HD void sc_mul(sc &r, const sc &a, const sc &b) {
  uint32_t p[16];
#pragma unroll
  for (int k = 0; k < 16; k++) p[k] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)a.w[i] * b.w[j] + p[i + j] + carry;
      p[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    p[i + 8] = (uint32_t)carry;
  }
  // 512 bits -> < 2^386 -> < 2^260 -> < 2^256 + 2^133 -> < 2^256
  uint32_t q1[13], q2[9], q3[9], q4[8];
  sc_fold<16, 13>(q1, p);
  sc_fold<13, 9>(q2, q1);
  sc_fold<9, 9>(q3, q2);
  sc_fold<9, 8>(q4, q3);  // q3[8] is 0 or 1, and q3[0..8) < 2^133 when it is 1
  sc_reduce_once(r, q4);
}

// r = a^(n-2) = 1/a mod n (0 for a = 0): square-and-multiply over the
// constant exponent, so every lane takes the same path.
TMV_HD void sc_inv(sc &r, const sc &a) {
  sc t;
#pragma unroll
  for (int k = 0; k < 8; k++) t.w[k] = k == 0 ? 1u : 0u;
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    sc_mul(t, t, t);
    const uint32_t word = (i >> 5) == 0 ? 0xD036413Fu : n_word(i >> 5);  // n - 2
    if ((word >> (i & 31)) & 1u) sc_mul(t, t, a);
  }
  r = t;
}
// 4-bit window i (0 = least significant) of a
TMV_HD uint32_t sc_nibble(const sc &a, int i) { return (a.w[i >> 3] >> (4 * (i & 7))) & 15u; }

// ------------------------------------------------------------------ group
// y^2 = x^3 + 7.  Affine points (x, y) and Jacobian points (X/Z^2, Y/Z^3) with
// an explicit infinity flag.  Coordinate magnitudes: X <= 6, Y <= 4, Z <= 2.
struct ge { fe x, y; };
struct gej { fe x, y, z; bool inf; };

TMV_HD void ge_generator(ge &g) {
  const uint32_t gx[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu, 0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
  const uint32_t gy[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u, 0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};
  fe_from_words(g.x, gx);
  fe_from_words(g.y, gy);
}
TMV_HD void gej_set_infinity(gej &r) {
  fe_set_int(r.x, 0);
  fe_set_int(r.y, 0);
  fe_set_int(r.z, 0);
  r.inf = true;
}
TMV_HD void gej_set_ge(gej &r, const ge &a) {
  r.x = a.x;
  r.y = a.y;
  fe_set_int(r.z, 1);
  r.inf = false;
}
TMV_HD void gej_cmov(gej &r, const gej &a, bool b) {
  fe_cmov(r.x, a.x, b);
  fe_cmov(r.y, a.y, b);
  fe_cmov(r.z, a.z, b);
  r.inf = b ? a.inf : r.inf;
}

// r = 2a (a = 0 curve: 3M + 4S).  X3 = 9X^4 - 8XY^2, Y3 = 3X^2 (12XY^2 -
// 9X^4) - 8Y^4, Z3 = 2YZ.  No point of the group has Y = 0, so the only
// special input is infinity, whose flag carries over.
TMV_HD void gej_double(gej &r, const gej &a) {
  SECP_ASSERT_MAG(a.x, 6);
  SECP_ASSERT_MAG(a.y, 4);
  SECP_ASSERT_MAG(a.z, 2);
  fe t1, t2, t3, t4, z3;
  fe_mul(z3, a.y, a.z);
  fe_mul_int(z3, z3, 2);  // 2
  fe_sq(t1, a.x);
  fe_mul_int(t1, t1, 3);  // 3: 3X^2
  fe_sq(t2, t1);          // 1: 9X^4
  fe_sq(t3, a.y);
  fe_mul_int(t3, t3, 2);  // 2: 2Y^2
  fe_sq(t4, t3);
  fe_mul_int(t4, t4, 2);  // 2: 8Y^4
  fe_mul(t3, t3, a.x);    // 1: 2XY^2
  fe x3, y3, u;
  fe_mul_int(x3, t3, 4);  // 4
  fe_neg(x3, x3, 4);      // 5
  fe_add(x3, x3, t2);     // 6
  fe_neg(t2, t2, 1);      // 2
  fe_mul_int(t3, t3, 6);  // 6
  fe_add(t3, t3, t2);     // 8: 12XY^2 - 9X^4
  fe_mul(y3, t1, t3);     // 1
  fe_neg(u, t4, 2);       // 3
  fe_add(y3, y3, u);      // 4
  r.x = x3;
  r.y = y3;
  r.z = z3;
  r.inf = a.inf;
}

// r = a + b for every pair: a == b goes to the doubling, a == -b to infinity,
// either operand may be infinity.  All candidates are computed and the result
// is chosen by conditional moves, so a wave never diverges here (the caller
// of an ECDSA verification chooses Q, r and s: every case is reachable).
// kAffineB: b.z is 1 (mixed addition: U1 = X1, S1 = Y1).
template <bool kAffineB>
TMV_HD void gej_add_any(gej &r, const gej &a, const gej &b) {
  SECP_ASSERT_MAG(a.x, 6);
  SECP_ASSERT_MAG(a.y, 4);
  SECP_ASSERT_MAG(a.z, 2);
  SECP_ASSERT_MAG(b.x, 6);
  SECP_ASSERT_MAG(b.y, 4);
  SECP_ASSERT_MAG(b.z, 2);
  fe z1z1, u1, u2, s1, s2, t, zz;
  fe_sq(z1z1, a.z);
  fe_mul(u2, b.x, z1z1);  // 1
  fe_mul(t, a.z, z1z1);
  fe_mul(s2, b.y, t);     // 1
  if (kAffineB) {
    u1 = a.x;             // 6
    s1 = a.y;             // 4
    zz = a.z;             // 2
  } else {
    fe z2z2;
    fe_sq(z2z2, b.z);
    fe_mul(u1, a.x, z2z2);  // 1
    fe_mul(t, b.z, z2z2);
    fe_mul(s1, a.y, t);     // 1
    fe_mul(zz, a.z, b.z);   // 1
  }
  const uint32_t mu = kAffineB ? 6 : 1, ms = kAffineB ? 4 : 1;
  fe h, rr, hh, hhh, v;
  fe_sub(h, u2, u1, mu);   // <= 8
  fe_sub(rr, s2, s1, ms);  // <= 6
  const bool h0 = fe_is_zero(h), r0 = fe_is_zero(rr);
  fe_sq(hh, h);
  fe_mul(hhh, h, hh);
  fe_mul(v, u1, hh);       // 1
  gej g;
  fe_sq(g.x, rr);          // 1
  fe_mul_int(t, v, 2);
  fe_add(t, t, hhh);       // 3
  fe_sub(g.x, g.x, t, 3);  // 5
  fe_sub(t, v, g.x, 5);    // 7
  fe_mul(g.y, rr, t);      // 1
  fe_mul(t, s1, hhh);      // 1
  fe_sub(g.y, g.y, t, 1);  // 3
  fe_mul(g.z, zz, h);      // 1
  g.inf = h0 && !r0;       // a == -b
  gej d;
  gej_double(d, a);
  gej_cmov(g, d, h0 && r0);  // a == b
  gej_cmov(g, a, b.inf);
  gej_cmov(g, b, a.inf);
  r = g;
}
TMV_HD void gej_add(gej &r, const gej &a, const gej &b) { gej_add_any<false>(r, a, b); }
TMV_HD void gej_add_ge(gej &r, const gej &a, const ge &b, bool b_inf) {
  gej bj;
  gej_set_ge(bj, b);
  bj.inf = b_inf;
  gej_add_any<true>(r, a, bj);
}

// Jacobian -> affine (host: table build, tests).  a must not be infinity.
TMV_HD void ge_set_gej(ge &r, const gej &a) {
  fe zi, zi2, zi3;
  fe_inv(zi, a.z);
  fe_sq(zi2, zi);
  fe_mul(zi3, zi2, zi);
  fe_mul(r.x, a.x, zi2);
  fe_mul(r.y, a.y, zi3);
  fe_normalize(r.x);
  fe_normalize(r.y);
}

// btcec ParsePubKey for the compressed form: prefix 0x02 / 0x03, x < p,
// y = (x^3 + 7)^((p+1)/4) with y^2 == x^3 + 7, y negated to the prefix's
// parity.  xw: x as 8 little-endian words.  On failure q is G (a valid point
// for the lanes that stay in the wave) and the result is false.
TMV_HD bool ge_decompress(ge &q, uint32_t prefix, const uint32_t xw[8]) {
  fe x, c, y, t;
  bool ok = fe_from_words_checked(x, xw);
  ok = ok && (prefix == 2 || prefix == 3);
  fe_sq(t, x);
  fe_mul(c, t, x);
  c.n[0] += 7;  // 2 (7 on a magnitude-1 limb)
  fe_sqrt_candidate(y, c);
  fe_sq(t, y);
  ok = ok && fe_equal(t, c, 2);
  fe_normalize(y);
  fe yn;
  fe_neg(yn, y, 1);  // 2
  fe_cmov(y, yn, fe_is_odd_normalized(y) != ((prefix & 1) != 0));
  ge g;
  ge_generator(g);
  q.x = x;
  q.y = y;
  fe_cmov(q.x, g.x, !ok);
  fe_cmov(q.y, g.y, !ok);
  return ok;
}

// ------------------------------------------------------------------ tables
// G table: entry j - 1 = j G, j = 1..15, affine and canonical, 20 words (x
// limbs, y limbs).  Built once by the host (context init) from this header.
constexpr int kWindowEntries = 15;
constexpr int kGTableWords = 20 * kWindowEntries;
// Q table of one signature: entry j = j Q, j = 1..15 (entry 0 unused),
// Jacobian, 32 words each (x, y, z limbs, two words of padding): 128-byte
// entries, so a lane reads whole cache lines.
constexpr int kQEntryWords = 32;
constexpr int kQTableWords = 16 * kQEntryWords;

inline void build_g_table(uint32_t *tab) {
  ge g;
  ge_generator(g);
  gej acc;
  gej_set_ge(acc, g);
  for (int j = 1; j <= kWindowEntries; j++) {
    ge a;
    ge_set_gej(a, acc);
    for (int i = 0; i < 10; i++) {
      tab[20 * (j - 1) + i] = a.x.n[i];
      tab[20 * (j - 1) + 10 + i] = a.y.n[i];
    }
    gej_add_ge(acc, acc, g, false);
  }
}

TMV_HD void store_fe(uint32_t *p, const fe &a) {
#pragma unroll
  for (int i = 0; i < 10; i++) p[i] = a.n[i];
}
TMV_HD void load_fe(fe &a, const uint32_t *p) {
#pragma unroll
  for (int i = 0; i < 10; i++) a.n[i] = p[i];
}

// qtab (kQTableWords words, 16-byte aligned) <- j Q, j = 1..15.  Each entry
// comes from the complete mixed addition, so 2Q is the doubling it selects.
TMV_HD void build_q_table(uint32_t *qtab, const ge &q) {
  gej acc;
  gej_set_ge(acc, q);
#pragma unroll 1
  for (int j = 1; j <= kWindowEntries; j++) {
    uint32_t *e = qtab + kQEntryWords * j;
    store_fe(e, acc.x);
    store_fe(e + 10, acc.y);
    store_fe(e + 20, acc.z);
    e[30] = 0;
    e[31] = 0;
    if (j < kWindowEntries) gej_add_ge(acc, acc, q, false);
  }
}

// ------------------------------------------------------------------ ECDSA verification
// What the chain needs of one signature (steps 1-6 of VerifySignature up to
// u1, u2): 32 words, the layout k_secp_prep writes and k_secp_verify reads.
struct VerifyInput {
  sc u1, u2;
  uint32_t r[8];     // r as little-endian words (1 <= r < n when ok)
  uint32_t ok;       // key parsed, lower-S, r and s in range
  uint32_t pad[7];
};

// Steps 2-6: parse, range tests, w = 1/s, u1 = z w, u2 = r w.  zw: SHA-256
// state words of the message (zw[0] most significant).  q: the key, or G when
// it does not parse.
TMV_HD void verify_prepare(VerifyInput &in, ge &q, uint32_t prefix, const uint32_t xw[8], const uint32_t rw[8],
                           const uint32_t sw[8], const uint32_t zw[8]) {
  bool ok = ge_decompress(q, prefix, xw);
  sc r, s, z, w;
  ok = sc_below_n(rw) && ok;
  ok = sc_below_n(sw) && ok;
  sc_reduce_once(r, rw);
  sc_reduce_once(s, sw);
  ok = ok && !sc_is_zero(r) && !sc_is_zero(s) && !sc_is_high(s);
  uint32_t zl[8];
#pragma unroll
  for (int k = 0; k < 8; k++) zl[k] = zw[7 - k];
  sc_reduce_once(z, zl);  // z < 2^256 < 2n
  sc_inv(w, s);
  sc_mul(in.u1, z, w);
  sc_mul(in.u2, r, w);
#pragma unroll
  for (int k = 0; k < 8; k++) in.r[k] = r.w[k];
  in.ok = ok ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 7; k++) in.pad[k] = 0;
}

// x(R') mod n == r for a Jacobian R' (steps 7-8): r Z^2 == X or, when
// r + n < p, (r + n) Z^2 == X.
TMV_HD bool verify_compare(const VerifyInput &in, const gej &acc) {
  // p - n = 0x14551231950b75fc4402da1722fc9baee: r + n < p iff r < p - n
  const uint32_t pmn[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u, 1u, 0u, 0u, 0u};
  uint32_t nw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nw[k] = n_word(k);
  fe fr, fn, z2, t;
  fe_from_words(fr, in.r);
  fe_from_words(fn, nw);
  fe_sq(z2, acc.z);
  fe_mul(t, fr, z2);               // 1
  bool match = fe_equal(acc.x, t, 1);
  fe_add(fr, fr, fn);              // 2: r + n, its true value when that is < p
  fe_mul(t, fr, z2);
  match = match || (words_less(in.r, pmn) && fe_equal(acc.x, t, 1));
  return in.ok != 0 && !acc.inf && match;
}

// Steps 6-8: R' = u1 G + u2 Q by interleaved 4-bit windows (Straus): 64 steps
// of four doublings, one mixed addition from the G table and one addition
// from the signature's Q table; then the compare.  gtab / qtab as above.
TMV_HD bool verify_chain(const VerifyInput &in, const uint32_t *gtab, const uint32_t *qtab) {
  gej acc;
  gej_set_infinity(acc);
#pragma unroll 1
  for (int i = 63; i >= 0; i--) {
#pragma unroll 1
    for (int k = 0; k < 4; k++) gej_double(acc, acc);
    const uint32_t d1 = sc_nibble(in.u1, i), d2 = sc_nibble(in.u2, i);
    ge g;
    const uint32_t *ge_ = gtab + 20 * (d1 ? d1 - 1 : 0);
    load_fe(g.x, ge_);
    load_fe(g.y, ge_ + 10);
    gej_add_ge(acc, acc, g, d1 == 0);
    gej qj;
    const uint32_t *qe = qtab + kQEntryWords * (d2 ? d2 : 1);
    load_fe(qj.x, qe);
    load_fe(qj.y, qe + 10);
    load_fe(qj.z, qe + 20);
    qj.inf = d2 == 0;
    gej_add(acc, acc, qj);
  }
  return verify_compare(in, acc);
}

// ------------------------------------------------------------------ comb tables
// A cached key Q (and, once per context, G) is kept as a 4-bit comb: the
// affine multiples d 16^j Q for window j = 0..63 and digit d = 1..15, so
// u Q = sum_j comb[j][nibble_j(u)] needs 64 mixed additions and no doublings.
// No entry is infinity: d 16^j <= 15 * 16^63 < n and Q has order n.  Entry
// (j, d) is 16 words at kCombEntryWords * (15 j + d - 1): x then y as 8
// little-endian words each, canonical (< p) -- 64 bytes, half a cache line,
// 61,440 bytes per key.
constexpr int kCombWindows = 64;
constexpr int kCombEntryWords = 16;
constexpr int kCombEntries = kCombWindows * kWindowEntries;   // 960
constexpr int kCombWords = kCombEntries * kCombEntryWords;    // 15,360
constexpr size_t kCombBytes = 4ull * kCombWords;              // 61,440

// out[16 k ...] <- pts[k] in affine form, k < n, with one inversion for all
// of them (Montgomery's trick: prefix products of the z, one fe_inv, and the
// walk back).  No point may be infinity.  pre: n field elements of scratch.
TMV_HD void comb_store_affine(uint32_t *out, const gej *pts, fe *pre, int n) {
  pre[0] = pts[0].z;
#pragma unroll 1
  for (int k = 1; k < n; k++) fe_mul(pre[k], pre[k - 1], pts[k].z);
  fe inv;
  fe_inv(inv, pre[n - 1]);  // 1 / (z_0 ... z_{n-1})
#pragma unroll 1
  for (int k = n - 1; k >= 0; k--) {
    fe zi, zi2, zi3, x, y;
    if (k) {
      fe_mul(zi, inv, pre[k - 1]);  // 1 / z_k
      fe_mul(inv, inv, pts[k].z);   // 1 / (z_0 ... z_{k-1})
    } else {
      zi = inv;
    }
    fe_sq(zi2, zi);
    fe_mul(zi3, zi2, zi);
    fe_mul(x, pts[k].x, zi2);
    fe_mul(y, pts[k].y, zi3);
    fe_normalize(x);
    fe_normalize(y);
    fe_to_words_normalized(out + kCombEntryWords * k, x);
    fe_to_words_normalized(out + kCombEntryWords * k + 8, y);
  }
}

// pts[0..15) <- d base, d = 1..15.  Each step is the complete addition: 2 base
// is the doubling it selects.
TMV_HD void comb_window_multiples(gej *pts, const gej &base) {
  pts[0] = base;
#pragma unroll 1
  for (int d = 1; d < kWindowEntries; d++) gej_add_any<false>(pts[d], pts[d - 1], base);
}

// The whole comb of q on one thread, one inversion per key (host: the G comb
// at context init, the tests; the device builds one window per lane,
// k_secp_key_table).  tab: kCombWords words.
inline void build_comb(uint32_t *tab, const ge &q) {
  gej *pts = new gej[kCombEntries];
  fe *pre = new fe[kCombEntries];
  gej base;
  gej_set_ge(base, q);
  for (int j = 0; j < kCombWindows; j++) {
    comb_window_multiples(pts + kWindowEntries * j, base);
    for (int k = 0; k < 4; k++) gej_double(base, base);
  }
  comb_store_affine(tab, pts, pre, kCombEntries);
  delete[] pts;
  delete[] pre;
}

// Comb entry (j, d) as an addend; d = 0 reads entry (j, 1) and is flagged
// infinity, so every lane loads 64 bytes whatever its digit.
TMV_HD void comb_load(gej &b, const uint32_t *tab, int j, uint32_t d) {
  const uint32_t *e = static_cast<const uint32_t *>(
      __builtin_assume_aligned(tab + kCombEntryWords * (kWindowEntries * j + (int)(d ? d - 1 : 0)), 16));
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = e[k];
  fe_from_words(b.x, w);
  fe_from_words(b.y, w + 8);
  fe_set_int(b.z, 1);
  b.inf = d == 0;
}

// Steps 2-6 without the key work (k_secp_prep_cached): the range tests,
// w = 1/s, u1 = z w, u2 = r w.  key_ok: the key parsed and has a comb.
TMV_HD void verify_prepare_cached(VerifyInput &in, bool key_ok, const uint32_t rw[8], const uint32_t sw[8],
                                  const uint32_t zw[8]) {
  sc r, s, z, w;
  bool ok = sc_below_n(rw) && key_ok;
  ok = sc_below_n(sw) && ok;
  sc_reduce_once(r, rw);
  sc_reduce_once(s, sw);
  ok = ok && !sc_is_zero(r) && !sc_is_zero(s) && !sc_is_high(s);
  uint32_t zl[8];
#pragma unroll
  for (int k = 0; k < 8; k++) zl[k] = zw[7 - k];
  sc_reduce_once(z, zl);  // z < 2^256 < 2n
  sc_inv(w, s);
  sc_mul(in.u1, z, w);
  sc_mul(in.u2, r, w);
#pragma unroll
  for (int k = 0; k < 8; k++) in.r[k] = r.w[k];
  in.ok = ok ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 7; k++) in.pad[k] = 0;
}

// R' = u1 G + u2 Q from the two combs: 128 complete mixed additions, window 63
// first, G's entry then Q's, and no doublings of the accumulator.  The caller
// of a verification chooses Q, r and s, so the accumulator can meet its own
// addend (Q = G with equal leading digits), its negative, or infinity:
// gej_add_any<true> takes every case by conditional moves.  rec: the
// signature's VerifyInput record in memory (32 words).  The digits are read
// from it window by window and r only for the compare, so the accumulator is
// all a lane keeps in registers and nothing of it is indexed at run time.
TMV_HD bool verify_chain_comb(const uint32_t *rec, const uint32_t *gcomb, const uint32_t *qcomb) {
  gej acc;
  gej_set_infinity(acc);
#pragma unroll 1
  for (int j = kCombWindows - 1; j >= 0; j--) {
#pragma unroll 1
    for (int h = 0; h < 2; h++) {  // one copy of the addition's code
      const uint32_t d = (rec[8 * h + (j >> 3)] >> (4 * (j & 7))) & 15u;
      gej e;
      comb_load(e, h ? qcomb : gcomb, j, d);
      gej_add_any<true>(acc, acc, e);
    }
  }
  VerifyInput in;
#pragma unroll
  for (int k = 0; k < 8; k++) in.r[k] = rec[16 + k];
  in.ok = rec[24];
  return verify_compare(in, acc);
}

// SHA-256 of a message held in ordinary memory -> 8 state words
TMV_HD void sha256_words(uint32_t st[8], const uint8_t *msg, uint32_t len) {
  const uint32_t nblk = (len + 72) / 64, end = 64 * nblk;
  const uint64_t bits = (uint64_t)len * 8;
  sha256_init(st);
#pragma unroll 1
  for (uint32_t k = 0; k < nblk; k++) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t pos = 64 * k + 4 * q + j;
        uint32_t byte = 0;
        if (pos < len) byte = msg[pos];  // never past the message's end
        else if (pos == len) byte = 0x80;
        else if (pos >= end - 8) byte = (uint32_t)(bits >> (8 * (end - 1 - pos))) & 0xffu;
        word = (word << 8) | byte;
      }
      w[q] = word;
    }
    sha256_compress(st, w);
  }
}

// ecdsa.Verify with btcec's key parsing and Tendermint's lower-S rule, one
// signature, on the calling thread (host: the G and Q tables on the stack).
// z32: SHA-256 of the message.
inline bool secp256k1_verify(const uint8_t pk33[33], const uint8_t z32[32], const uint8_t sig64[64]) {
  static const struct GTable {
    uint32_t w[kGTableWords];
    GTable() { build_g_table(w); }
  } g;
  uint32_t xw[8], rw[8], sw[8], zl[8], zw[8];
  words_from_be32(xw, pk33 + 1);
  words_from_be32(rw, sig64);
  words_from_be32(sw, sig64 + 32);
  words_from_be32(zl, z32);
  for (int k = 0; k < 8; k++) zw[k] = zl[7 - k];
  VerifyInput in;
  ge q;
  verify_prepare(in, q, pk33[0], xw, rw, sw, zw);
  alignas(16) uint32_t qtab[kQTableWords];
  for (int k = 0; k < kQEntryWords; k++) qtab[k] = 0;
  build_q_table(qtab, q);
  return verify_chain(in, g.w, qtab);
}

// The same verdict through the combs, as the cached device path computes it
// (host: the tests of that path's arithmetic).  build_key_comb is
// k_secp_key_table's work for one key: false when the key does not parse (tab
// then holds G's comb, as a slot would); secp256k1_verify_comb is
// k_secp_prep_cached and k_secp_verify_comb for one signature.
inline const uint32_t *g_comb_host() {
  static const struct GComb {
    uint32_t *w;
    GComb() : w(new uint32_t[kCombWords]) {
      ge g;
      ge_generator(g);
      build_comb(w, g);
    }
    ~GComb() { delete[] w; }
  } g;
  return g.w;
}
inline bool build_key_comb(uint32_t *tab, const uint8_t pk33[33]) {
  uint32_t xw[8];
  words_from_be32(xw, pk33 + 1);
  ge q;
  const bool ok = ge_decompress(q, pk33[0], xw);
  build_comb(tab, q);
  return ok;
}
inline bool secp256k1_verify_comb(bool key_ok, const uint32_t *qcomb, const uint8_t z32[32], const uint8_t sig64[64]) {
  static_assert(sizeof(VerifyInput) == 128, "the record is 32 words");
  uint32_t rw[8], sw[8], zl[8], zw[8];
  words_from_be32(rw, sig64);
  words_from_be32(sw, sig64 + 32);
  words_from_be32(zl, z32);
  for (int k = 0; k < 8; k++) zw[k] = zl[7 - k];
  VerifyInput in;
  verify_prepare_cached(in, key_ok, rw, sw, zw);
  return verify_chain_comb(reinterpret_cast<const uint32_t *>(&in), g_comb_host(), qcomb);
}

// PubKey.VerifySignature(msg, sig) on the host (secp256k1.go:206-226)
inline bool secp256k1_verify_msg(const uint8_t *pk, size_t pk_len, const uint8_t *msg, size_t msg_len,
                                 const uint8_t *sig, size_t sig_len) {
  if (pk_len != 33 || sig_len != 64 || msg_len > 0x3fffffffu) return false;
  uint32_t st[8];
  sha256_words(st, msg, (uint32_t)msg_len);
  uint8_t z[32];
  for (int i = 0; i < 8; i++) {
    z[4 * i] = (uint8_t)(st[i] >> 24); z[4 * i + 1] = (uint8_t)(st[i] >> 16);
    z[4 * i + 2] = (uint8_t)(st[i] >> 8); z[4 * i + 3] = (uint8_t)st[i];
  }
  return secp256k1_verify(pk, z, sig);
}

}  // namespace secp
}  // namespace tmv
