// Host build of tendermint_amd/csrc/secp256k1.h with limb-bound assertions
// (-DTMV_BOUNDS_CHECK) behind a small C interface for
// tests/test_secp256k1_host.py.  Values cross as 32 big-endian bytes.
#include <cstring>

#include "../../../tendermint_amd/csrc/secp256k1.h"

using namespace tmv::secp;

namespace {

void fe_in(fe &r, const uint8_t *b) {
  uint32_t w[8];
  words_from_be32(w, b);
  fe_from_words(r, w);  // values >= p are taken as they are (magnitude 1)
}
void sc_in(sc &r, const uint8_t *b) {
  uint32_t w[8];
  words_from_be32(w, b);
  sc_reduce_once(r, w);
}
void sc_out(uint8_t *b, const sc &a) { words_to_be32(b, a.w); }

// affine (x, y) scaled to Jacobian (x l^2, y l^3, l); inf: infinity
void gej_in(gej &r, const uint8_t *x, const uint8_t *y, const uint8_t *l, int inf) {
  fe fx, fy, fl, l2, l3;
  fe_in(fx, x);
  fe_in(fy, y);
  fe_in(fl, l);
  fe_sq(l2, fl);
  fe_mul(l3, l2, fl);
  fe_mul(r.x, fx, l2);
  fe_mul(r.y, fy, l3);
  r.z = fl;
  r.inf = inf != 0;
}
int gej_out(uint8_t *x, uint8_t *y, const gej &a) {
  if (a.inf) return 1;
  ge g;
  ge_set_gej(g, a);
  fe_to_be32(x, g.x);
  fe_to_be32(y, g.y);
  return 0;
}

}  // namespace

extern "C" {

// op: 0 mul, 1 sq, 2 add, 3 sub, 4 neg, 5 sqrt candidate, 6 inverse, 7 normalise
void secpcheck_fe_op(int op, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  fe x, y, r;
  fe_in(x, a);
  fe_in(y, b);
  switch (op) {
    case 0: fe_mul(r, x, y); break;
    case 1: fe_sq(r, x); break;
    case 2: fe_add(r, x, y); break;
    case 3: fe_sub(r, x, y, 1); break;
    case 4: fe_neg(r, x, 1); break;
    case 5: fe_sqrt_candidate(r, x); break;
    case 6: fe_inv(r, x); break;
    default: r = x; break;
  }
  fe_to_be32(out, r);
}

// a chain of dependent steps at the largest magnitudes the formulas use:
// t <- (3 t - a)^2 * (t + 5 a) + a, `steps` times, never normalised on the way
void secpcheck_fe_chain(const uint8_t *a, const uint8_t *t0, int steps, uint8_t *out) {
  fe x, t;
  fe_in(x, a);
  fe_in(t, t0);
  for (int i = 0; i < steps; i++) {
    fe u, v, w;
    fe_mul_int(u, t, 3);   // 6 (t: <= 2)
    fe_sub(u, u, x, 1);    // 8
    fe_sq(u, u);           // 1
    fe_mul_int(v, x, 5);   // 5
    fe_add(w, t, v);       // 7
    fe_mul(v, u, w);       // 1
    fe_add(t, v, x);       // 2
  }
  fe_to_be32(out, t);
}

// 1 when a and b are equal mod p (a taken at magnitude 1, b through a negation)
int secpcheck_fe_equal(const uint8_t *a, const uint8_t *b) {
  fe x, y;
  fe_in(x, a);
  fe_in(y, b);
  return fe_equal(x, y, 1) ? 1 : 0;
}
int secpcheck_fe_from_be32(const uint8_t *a, uint8_t *out) {
  fe x;
  const bool ok = fe_from_be32(x, a);
  fe_to_be32(out, x);
  return ok ? 1 : 0;
}

// op: 0 mul, 1 inverse; returns flags of a: bit 0 below n, bit 1 zero, bit 2 high
int secpcheck_sc_op(int op, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  sc x, y, r;
  const bool below = sc_from_be32(x, a);
  sc_in(y, b);
  if (op == 0) sc_mul(r, x, y);
  else sc_inv(r, x);
  sc_out(out, r);
  return (below ? 1 : 0) | (sc_is_zero(x) ? 2 : 0) | (sc_is_high(x) ? 4 : 0);
}

// op 0: a + b (complete addition), 1: a + b with b affine (lb ignored),
// 2: 2a.  Returns 1 when the result is infinity, else writes it (affine).
int secpcheck_group_op(int op, const uint8_t *ax, const uint8_t *ay, const uint8_t *la, int a_inf, const uint8_t *bx,
                       const uint8_t *by, const uint8_t *lb, int b_inf, uint8_t *ox, uint8_t *oy) {
  gej a, b, r;
  gej_in(a, ax, ay, la, a_inf);
  if (op == 0) {
    gej_in(b, bx, by, lb, b_inf);
    gej_add(r, a, b);
  } else if (op == 1) {
    ge g;
    fe_in(g.x, bx);
    fe_in(g.y, by);
    gej_add_ge(r, a, g, b_inf != 0);
  } else {
    gej_double(r, a);
  }
  return gej_out(ox, oy, r);
}

// btcec ParsePubKey: 1 and (x, y) when pk33 parses
int secpcheck_decompress(const uint8_t *pk33, uint8_t *ox, uint8_t *oy) {
  uint32_t xw[8];
  words_from_be32(xw, pk33 + 1);
  ge q;
  const bool ok = ge_decompress(q, pk33[0], xw);
  fe_to_be32(ox, q.x);
  fe_to_be32(oy, q.y);
  return ok ? 1 : 0;
}

void secpcheck_g_table(uint32_t *out) { build_g_table(out); }

int secpcheck_verify(const uint8_t *pk33, const uint8_t *z32, const uint8_t *sig64) {
  return secp256k1_verify(pk33, z32, sig64) ? 1 : 0;
}
int secpcheck_verify_msg(const uint8_t *pk, size_t pk_len, const uint8_t *msg, size_t msg_len, const uint8_t *sig,
                         size_t sig_len) {
  return secp256k1_verify_msg(pk, pk_len, msg, msg_len, sig, sig_len) ? 1 : 0;
}
}
