// Engine double for the vote-extension host layer
// (csrc/host/tm_vote_ext_abi.cpp): the entry points of include/tmverify.h
// that file calls, on the host.  Messages are assembled with the product's
// host encoder (vote_ext_encode.h, tm_types.h) from the templates and payloads
// the host layer sends, and each signature's status comes from
// voteext_status, which the including program defines (the C oracle in
// voteextcheck.cpp, a keyed hash in voteext_san.cpp).  Included by exactly one
// translation unit of a program.
#pragma once
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "host/tm_types.h"
#include "host/vote_ext_encode.h"

struct tmv_ctx {
  int unused;
};

// 1 valid, 0 invalid (sr25519: < 0 undecodable key / signature)
int8_t voteext_status(uint8_t kind, const uint8_t *pk, const uint8_t *msg, size_t mlen, const uint8_t *sig);

extern "C" {

std::atomic<int> voteext_calls_host_built{0};    // tmv_verify_batch_ex
std::atomic<int> voteext_calls_device_built{0};  // tmv_verify_votes_and_extensions
std::atomic<int> voteext_entries{0};

static thread_local std::string g_double_error;
const char *tmv_last_error(void) { return g_double_error.c_str(); }
void tmv_internal_set_error(const char *msg) { g_double_error = msg ? msg : ""; }

int tmv_verify_batch_ex(tmv_ctx *, uint8_t key_kind, uint32_t, const uint8_t *pk, const uint8_t *sig,
                        const uint8_t *msg, const uint32_t *msg_off, uint32_t n, int8_t *status_out) {
  voteext_calls_host_built++;
  voteext_entries += (int)n;
  bool all = n > 0;
  for (uint32_t i = 0; i < n; i++) {
    status_out[i] = voteext_status(key_kind, pk + 32 * i, msg + msg_off[i], msg_off[i + 1] - msg_off[i], sig + 64 * i);
    all = all && status_out[i] == 1;
  }
  return all ? TMV_ALL_VALID : TMV_NOT_ALL;
}

int tmv_verify_votes_and_extensions(tmv_ctx *, uint8_t key_kind, uint32_t, const tmv_vote_template *tmpl,
                                    uint32_t n_tmpl, const tmv_vote *votes, uint32_t n_votes,
                                    const tmv_vote_ext_template *etmpl, uint32_t n_etmpl, const uint32_t *ext_tmpl,
                                    const uint8_t *ext_data, const uint32_t *ext_off, uint32_t n_exts,
                                    const uint8_t *pk, const uint8_t *sig, int8_t *status_out) {
  voteext_calls_device_built++;
  voteext_entries += (int)(n_votes + n_exts);
  if (n_exts && ext_off[0] != 0) return TMV_ERR_ARG;
  bool all = n_votes + n_exts > 0;
  for (uint32_t i = 0; i < n_votes + n_exts; i++) {
    tmh::Bytes m;
    if (i < n_votes) {
      const uint32_t t = votes[i].tmpl & ~TMV_VOTE_WITH_BLOCK;
      if (t >= n_tmpl) return TMV_ERR_ARG;
      tmh::VoteTemplate vt;
      vt.head_len = tmpl[t].head_len, vt.block_len = tmpl[t].block_len, vt.chain_len = tmpl[t].chain_len;
      vt.bytes.insert(vt.bytes.end(), tmpl[t].head, tmpl[t].head + tmpl[t].head_len);
      vt.bytes.insert(vt.bytes.end(), tmpl[t].block, tmpl[t].block + tmpl[t].block_len);
      vt.bytes.insert(vt.bytes.end(), tmpl[t].chain, tmpl[t].chain + tmpl[t].chain_len);
      tmh::AppendVoteFromTemplate(m, vt, (votes[i].tmpl & TMV_VOTE_WITH_BLOCK) != 0,
                                  tmh::Timestamp{votes[i].ts_seconds, votes[i].ts_nanos});
    } else {
      const uint32_t j = i - n_votes;
      if (ext_tmpl[j] >= n_etmpl || ext_off[j + 1] < ext_off[j]) return TMV_ERR_ARG;
      tmh::AppendVoteExtFromTail(m, etmpl[ext_tmpl[j]].tail, etmpl[ext_tmpl[j]].tail_len, ext_data + ext_off[j],
                                 ext_off[j + 1] - ext_off[j]);
    }
    status_out[i] = voteext_status(key_kind, pk + 32 * i, m.data(), m.size(), sig + 64 * i);
    all = all && status_out[i] == 1;
  }
  return all ? TMV_ALL_VALID : TMV_NOT_ALL;
}

}  // extern "C"
