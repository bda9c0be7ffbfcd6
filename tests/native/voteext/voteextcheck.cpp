// The vote-extension host layer (csrc/host/tm_vote_ext_abi.cpp) without the
// engine, for tests/test_vote_ext_host.py: the engine double of
// engine_double.h with the C oracle's signature checks, the host layer's entry
// point over a context of the double, and the device's length functions
// (csrc/vote_ext.h, host build) for the host / device agreement test.
#include <cstring>

#include "engine_double.h"
#include "host/ripemd160.h"
#include "vote_ext.h"

extern "C" {
int oracle_ed25519_verify(const uint8_t *pk, const uint8_t *msg, size_t mlen, const uint8_t *sig);
int oracle_sr25519_add_check(const uint8_t *pk, const uint8_t *sig);
int oracle_sr25519_verify(const uint8_t *pk, const uint8_t *msg, size_t mlen, const uint8_t *sig);
}

int8_t voteext_status(uint8_t kind, const uint8_t *pk, const uint8_t *msg, size_t mlen, const uint8_t *sig) {
  static const uint8_t none = 0;
  if (!msg) msg = &none;
  if (kind == TMV_KIND_SR25519) {
    const int a = oracle_sr25519_add_check(pk, sig);  // 0 ok, -1 key, -2 signature
    if (a < 0) return (int8_t)a;
    return (int8_t)oracle_sr25519_verify(pk, msg, mlen, sig);
  }
  return (int8_t)oracle_ed25519_verify(pk, msg, mlen, sig);
}

static tmv_ctx g_ctx;

extern "C" {

int voteext_verify_extended_votes(int mode, const char *chain_id, const tmv_ext_vote_in *votes, uint32_t n,
                                  int32_t *results, uint8_t *failed_sig) {
  return tmv_verify_extended_votes(&g_ctx, mode, chain_id, votes, n, results, failed_sig);
}

// the device's sizing of one extension message (k_vote_ext_signbytes)
uint32_t voteext_device_msg_len(uint32_t tail_len, uint32_t ext_len) { return tmv::vote_ext_msg_len(tail_len, ext_len); }
uint32_t voteext_device_wave_min(void) { return tmv::kVoteExtWaveMin; }

void voteext_ripemd160(const uint8_t *msg, size_t len, uint8_t out[20]) { tmh::Ripemd160(msg, len, out); }

}  // extern "C"
