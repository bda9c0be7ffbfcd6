// Vote extensions of the host layer (include/tmhost.h):
//   tmv_vote_extension_sign_bytes       types.VoteExtensionSignBytes (types/vote.go:159-172)
//   tmv_vote_extension_template_encode  the template of tmv_verify_votes_and_extensions
//   tmv_verify_extended_votes           Vote.Verify / VerifyVoteAndExtension / VerifyExtension
//                                       (types/vote.go:226-276) of many votes at once
// The vote and extension signatures of a call go out together, one engine
// call per key kind.  The engine's extension entry and its secp256k1 entry
// are weak references, as tm_block_abi.cpp's: a build of this file without
// them loads all the same and sends host-built messages
// (vote_ext_encode.h) through tmv_verify_batch_ex, the same verdicts.  Only
// the public tmv_* C-ABI is used to reach the device (layering).
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "../secp256k1.h"
#include "ripemd160.h"
#include "tm_host_internal.h"
#include "tm_light.h"
#include "vote_ext_encode.h"

extern "C" int tmv_verify_votes_and_extensions(tmv_ctx *ctx, uint8_t key_kind, uint32_t flags,
                                               const tmv_vote_template *tmpl, uint32_t n_tmpl, const tmv_vote *votes,
                                               uint32_t n_votes, const tmv_vote_ext_template *etmpl, uint32_t n_etmpl,
                                               const uint32_t *ext_tmpl, const uint8_t *ext_data,
                                               const uint32_t *ext_off, uint32_t n_exts, const uint8_t *pk,
                                               const uint8_t *sig, int8_t *status_out) __attribute__((weak));
extern "C" int tmv_secp256k1_verify_batch(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg,
                                          const uint32_t *msg_off, uint32_t n, uint8_t *valid_out)
    __attribute__((weak));
extern "C" int tmv_secp256k1_verify_batch_ex(tmv_ctx *ctx, uint32_t flags, const uint8_t *pk, const uint8_t *sig,
                                             const uint8_t *msg, const uint32_t *msg_off, uint32_t n,
                                             uint8_t *valid_out) __attribute__((weak));

namespace {

using tmh::Bytes;
using tmh_internal::parallel_for;

// Signatures of one key kind in a call from which that kind's messages are
// built on the device (TMV_VOTE_EXT_DEVICE_MIN; tmhost.h has the default and
// DESIGN.md section 17 what it rests on).  Read on every call: tests change it.
uint32_t device_min() {
  const char *e = std::getenv("TMV_VOTE_EXT_DEVICE_MIN");
  return e ? (uint32_t)std::strtoul(e, nullptr, 10) : TMV_VOTE_EXT_DEVICE_MIN_DEFAULT;
}

tmh::BlockID block_id_of(const tmv_block_id &b) {
  tmh::BlockID r;
  if (b.hash && b.hash_len) r.hash.assign(b.hash, b.hash + b.hash_len);
  r.part_set_header.total = b.psh_total;
  if (b.psh_hash && b.psh_hash_len) r.part_set_header.hash.assign(b.psh_hash, b.psh_hash + b.psh_hash_len);
  return r;
}

bool block_is_nil(const tmv_block_id *b) { return !b || (b->hash_len == 0 && b->psh_total == 0 && b->psh_hash_len == 0); }

bool same_bytes(const uint8_t *a, uint32_t al, const uint8_t *b, uint32_t bl) {
  return al == bl && (al == 0 || std::memcmp(a, b, al) == 0);
}

// Two votes whose sign-bytes share everything but the timestamp.
bool same_vote_template(const tmv_vote_in &a, const tmv_vote_in &b) {
  if (a.type != b.type || a.height != b.height || a.round != b.round) return false;
  const bool an = block_is_nil(a.block_id), bn = block_is_nil(b.block_id);
  if (an || bn) return an && bn;
  const tmv_block_id &x = *a.block_id, &y = *b.block_id;
  return x.psh_total == y.psh_total && same_bytes(x.hash, x.hash_len, y.hash, y.hash_len) &&
         same_bytes(x.psh_hash, x.psh_hash_len, y.psh_hash, y.psh_hash_len);
}

// PubKey.Address(): SHA-256(key)[:20] (crypto.AddressHash; ed25519, sr25519),
// RIPEMD160(SHA256(key)) for secp256k1 (crypto/secp256k1/secp256k1.go).
void address_of(uint8_t kind, const uint8_t *pk, uint32_t pk_len, uint8_t addr[20]) {
  static const uint8_t none = 0;
  uint32_t st[8];
  tmh::Sha256Bytes(st, nullptr, 0, pk ? pk : &none, pk ? pk_len : 0);
  uint8_t dg[32];
  for (int k = 0; k < 32; k++) dg[k] = (uint8_t)(st[k / 4] >> (24 - 8 * (k % 4)));
  if (kind == TMV_KIND_SECP256K1) tmh::Ripemd160(dg, 32, addr);
  else std::memcpy(addr, dg, 20);
}

// One signature to verify: vote v's own (ext = false) or its extension's.
struct Entry {
  uint32_t v;
  bool ext;
};

// Per vote: which of its two signatures are to be checked, and which of them
// already failed without the engine (wrong lengths, unsupported key).
struct Need {
  bool vote = false, ext = false;
  uint8_t cls = 255;  // key kind of the entries sent to the engine; 255 = none
};

}  // namespace

extern "C" {

size_t tmv_vote_extension_sign_bytes(const char *chain_id, int64_t height, int32_t round, const uint8_t *ext,
                                     size_t ext_len, uint8_t *out, size_t cap) {
  Bytes b;
  tmh::AppendVoteExtSignBytes(b, chain_id ? chain_id : "", height, round, ext, ext ? ext_len : 0);
  if (out && cap) std::memcpy(out, b.data(), std::min(cap, b.size()));
  return b.size();
}

size_t tmv_vote_extension_template_encode(const char *chain_id, int64_t height, int32_t round, uint8_t *out,
                                          size_t cap) {
  const Bytes t = tmh::EncodeVoteExtTail(chain_id ? chain_id : "", height, round);
  if (out && cap && !t.empty()) std::memcpy(out, t.data(), std::min(cap, t.size()));
  return t.size();
}

int tmv_verify_extended_votes(tmv_ctx *ctx, int mode, const char *chain_id, const tmv_ext_vote_in *votes, uint32_t n,
                              int32_t *results, uint8_t *failed_sig) {
  if (!ctx || (n && (!votes || !results)) || mode < TMV_VOTE_MODE_VERIFY || mode > TMV_VOTE_MODE_EXTENSION)
    return TMV_ERR_ARG;
  const std::string chain = chain_id ? chain_id : "";
  // What the reference would look at, vote by vote: the address (not in
  // VerifyExtension), the vote signature (not in VerifyExtension), the
  // extension signature (non-nil precommits, not in Verify).  VerifySignature
  // semantics: a wrong key or signature length is an invalid signature.
  std::vector<Need> need(n);
  std::vector<uint8_t> vote_ok(n, 0), ext_ok(n, 0);  // 1 once the engine says so
  parallel_for(n, 256, [&](size_t i) {
    const tmv_ext_vote_in &x = votes[i];
    const tmv_vote_in &v = x.vote;
    results[i] = TMV_VOTE_OK;
    if (mode != TMV_VOTE_MODE_EXTENSION) {
      uint8_t addr[20];
      address_of(v.key_kind, v.pub_key, v.pub_key_len, addr);
      if (v.validator_address_len != 20 || !v.validator_address || std::memcmp(addr, v.validator_address, 20) != 0) {
        results[i] = TMV_VOTE_ERR_INVALID_ADDRESS;
        return;
      }
    }
    Need &nd = need[i];
    const bool key_ok = v.pub_key && ((v.key_kind == TMV_KIND_ED25519 || v.key_kind == TMV_KIND_SR25519)
                                          ? v.pub_key_len == 32
                                          : v.key_kind == TMV_KIND_SECP256K1 && v.pub_key_len == 33);
    const bool want_vote = mode != TMV_VOTE_MODE_EXTENSION;
    const bool want_ext = mode != TMV_VOTE_MODE_VERIFY && v.type == tmh::kPrecommitType && !block_is_nil(v.block_id);
    if (key_ok) nd.cls = v.key_kind;
    nd.vote = want_vote && key_ok && v.signature && v.signature_len == 64;
    nd.ext = want_ext && key_ok && x.extension_signature && x.extension_signature_len == 64 &&
             (x.extension || x.extension_len == 0);
    // signatures that need no engine to be wrong
    if (want_vote && !nd.vote) nd.ext = false;  // the reference stops at the vote signature
    vote_ok[i] = !want_vote;
    ext_ok[i] = !want_ext;
  });

  for (uint8_t k : {(uint8_t)TMV_KIND_ED25519, (uint8_t)TMV_KIND_SR25519, (uint8_t)TMV_KIND_SECP256K1}) {
    // entries of this kind: the vote signatures, then the extension signatures
    std::vector<Entry> ents;
    for (uint32_t i = 0; i < n; i++)
      if (need[i].cls == k && need[i].vote) ents.push_back(Entry{i, false});
    const size_t nv = ents.size();
    for (uint32_t i = 0; i < n; i++)
      if (need[i].cls == k && need[i].ext) ents.push_back(Entry{i, true});
    const size_t m = ents.size(), ne = m - nv;
    if (m == 0) continue;
    const size_t pkl = k == TMV_KIND_SECP256K1 ? 33 : 32;
    std::vector<uint8_t> pk(pkl * m), sig(64 * m);
    parallel_for(m, 512, [&](size_t t) {
      const tmv_ext_vote_in &x = votes[ents[t].v];
      std::memcpy(&pk[pkl * t], x.vote.pub_key, pkl);
      std::memcpy(&sig[64 * t], ents[t].ext ? x.extension_signature : x.vote.signature, 64);
    });
    std::vector<int8_t> st(m, 0);
    const bool on_device = k != TMV_KIND_SECP256K1 && tmv_verify_votes_and_extensions && m >= device_min();
    if (on_device) {
      // templates: the votes' shared fields per (type, height, round, block),
      // the extensions' tails per (height, round); consecutive votes usually
      // share theirs, so the last key is compared before the map is asked
      std::vector<tmh::VoteTemplate> vt;
      std::vector<tmv_vote> dv(nv);
      std::unordered_map<std::string, uint32_t> vmap, emap;
      const tmv_vote_in *last = nullptr;
      uint32_t last_idx = 0;
      for (size_t t = 0; t < nv; t++) {
        const tmv_vote_in &v = votes[ents[t].v].vote;
        const bool nil = block_is_nil(v.block_id);
        if (last && same_vote_template(*last, v)) {
          dv[t] = tmv_vote{v.ts_seconds, v.ts_nanos, last_idx | (nil ? 0u : TMV_VOTE_WITH_BLOCK)};
          continue;
        }
        std::string key(reinterpret_cast<const char *>(&v.type), sizeof v.type);
        key.append(reinterpret_cast<const char *>(&v.height), sizeof v.height);
        key.append(reinterpret_cast<const char *>(&v.round), sizeof v.round);
        if (!nil) {
          const tmv_block_id &b = *v.block_id;
          key.append(reinterpret_cast<const char *>(&b.hash_len), sizeof b.hash_len);
          if (b.hash_len) key.append(reinterpret_cast<const char *>(b.hash), b.hash_len);
          key.append(reinterpret_cast<const char *>(&b.psh_total), sizeof b.psh_total);
          if (b.psh_hash_len) key.append(reinterpret_cast<const char *>(b.psh_hash), b.psh_hash_len);
        }
        auto it = vmap.find(key);
        if (it == vmap.end()) {
          tmh::BlockID bid;
          if (!nil) bid = block_id_of(*v.block_id);
          vt.push_back(tmh::EncodeVoteTemplate(chain, v.type, v.height, v.round, nil ? nullptr : &bid));
          it = vmap.emplace(std::move(key), (uint32_t)vt.size() - 1).first;
        }
        last_idx = it->second;
        last = &v;
        dv[t] = tmv_vote{v.ts_seconds, v.ts_nanos, last_idx | (nil ? 0u : TMV_VOTE_WITH_BLOCK)};
      }
      std::vector<tmv_vote_template> ct(vt.size());
      for (size_t t = 0; t < vt.size(); t++) {
        const uint8_t *b = vt[t].bytes.data();
        ct[t] = tmv_vote_template{b, vt[t].head_len, b + vt[t].head_len, vt[t].block_len,
                                  b + vt[t].head_len + vt[t].block_len, vt[t].chain_len};
      }
      std::vector<Bytes> tails;
      std::vector<uint32_t> etmpl(ne), eoff(ne + 1, 0);
      const tmv_vote_in *elast = nullptr;
      for (size_t t = 0; t < ne; t++) {
        const tmv_ext_vote_in &x = votes[ents[nv + t].v];
        if (!elast || elast->height != x.vote.height || elast->round != x.vote.round) {
          std::string key(reinterpret_cast<const char *>(&x.vote.height), sizeof x.vote.height);
          key.append(reinterpret_cast<const char *>(&x.vote.round), sizeof x.vote.round);
          auto it = emap.find(key);
          if (it == emap.end()) {
            tails.push_back(tmh::EncodeVoteExtTail(chain, x.vote.height, x.vote.round));
            it = emap.emplace(std::move(key), (uint32_t)tails.size() - 1).first;
          }
          last_idx = it->second;
          elast = &x.vote;
        }
        etmpl[t] = last_idx;
        const uint64_t end = (uint64_t)eoff[t] + x.extension_len;
        if (end > UINT32_MAX) { tmv_internal_set_error("vote extensions exceed 4 GiB"); return TMV_ERR_ARG; }
        eoff[t + 1] = (uint32_t)end;
      }
      std::vector<uint8_t> edata(std::max<size_t>(eoff[ne], 1));
      parallel_for(ne, 512, [&](size_t t) {
        const tmv_ext_vote_in &x = votes[ents[nv + t].v];
        if (x.extension_len) std::memcpy(&edata[eoff[t]], x.extension, x.extension_len);
      });
      std::vector<tmv_vote_ext_template> cet(tails.size());
      for (size_t t = 0; t < tails.size(); t++) cet[t] = tmv_vote_ext_template{tails[t].data(), (uint32_t)tails[t].size()};
      const int rc = tmv_verify_votes_and_extensions(ctx, k, TMV_FLAG_KEY_CACHE, ct.data(), (uint32_t)ct.size(),
                                                     dv.data(), (uint32_t)nv, cet.data(), (uint32_t)cet.size(),
                                                     etmpl.data(), edata.data(), eoff.data(), (uint32_t)ne, pk.data(),
                                                     sig.data(), st.data());
      if (rc < 0) return rc;
    } else {
      // host-built messages: the extensions' tail once per (height, round) run
      // (and the votes' shared fields once per run of one block), the entries
      // cut into pieces that the worker pool encodes side by side
      const size_t pieces = std::max<size_t>(1, std::min<size_t>(64, m / 1024));
      std::vector<Bytes> part(pieces);
      std::vector<uint64_t> end(m);  // message ends inside the entry's piece
      parallel_for(pieces, 1, [&](size_t c) {
        const size_t lo = m * c / pieces, hi = m * (c + 1) / pieces;
        Bytes &out = part[c], tail;
        tmh::VoteTemplate vt;
        const tmv_vote_in *tv = nullptr, *te = nullptr;  // the votes vt / tail were encoded from
        for (size_t t = lo; t < hi; t++) {
          const tmv_ext_vote_in &x = votes[ents[t].v];
          const tmv_vote_in &v = x.vote;
          if (!ents[t].ext) {
            const bool nil = block_is_nil(v.block_id);
            if (!tv || !same_vote_template(*tv, v)) {
              tmh::BlockID bid;
              if (!nil) bid = block_id_of(*v.block_id);
              vt = tmh::EncodeVoteTemplate(chain, v.type, v.height, v.round, nil ? nullptr : &bid);
              tv = &v;
            }
            tmh::AppendVoteFromTemplate(out, vt, !nil, tmh::Timestamp{v.ts_seconds, v.ts_nanos});
          } else {
            if (!te || te->height != v.height || te->round != v.round) {
              tail = tmh::EncodeVoteExtTail(chain, v.height, v.round);
              te = &v;
            }
            tmh::AppendVoteExtFromTail(out, tail.data(), tail.size(), x.extension, x.extension_len);
          }
          end[t] = out.size();
        }
      });
      uint64_t total = 0;
      std::vector<uint64_t> base(pieces);
      for (size_t c = 0; c < pieces; c++) {
        base[c] = total;
        total += part[c].size();
      }
      if (total > UINT32_MAX) { tmv_internal_set_error("vote messages exceed 4 GiB"); return TMV_ERR_ARG; }
      Bytes msg(std::max<uint64_t>(total, 1));
      std::vector<uint32_t> off(m + 1, 0);
      parallel_for(pieces, 1, [&](size_t c) {
        const size_t lo = m * c / pieces, hi = m * (c + 1) / pieces;
        if (!part[c].empty()) std::memcpy(msg.data() + base[c], part[c].data(), part[c].size());
        for (size_t t = lo; t < hi; t++) off[t + 1] = (uint32_t)(base[c] + end[t]);
      });
      if (k != TMV_KIND_SECP256K1) {
        const int rc = tmv_verify_batch_ex(ctx, k, TMV_FLAG_KEY_CACHE, pk.data(), sig.data(), msg.data(), off.data(),
                                           (uint32_t)m, st.data());
        if (rc < 0) return rc;
      } else if (tmv_secp256k1_verify_batch_ex || tmv_secp256k1_verify_batch) {  // the device entry (libtmgpu.so: always)
        std::vector<uint8_t> valid(m, 0);
        const int rc = tmv_secp256k1_verify_batch_ex  // validators' keys cached
                           ? tmv_secp256k1_verify_batch_ex(ctx, TMV_FLAG_KEY_CACHE, pk.data(), sig.data(), msg.data(),
                                                           off.data(), (uint32_t)m, valid.data())
                           : tmv_secp256k1_verify_batch(ctx, pk.data(), sig.data(), msg.data(), off.data(),
                                                        (uint32_t)m, valid.data());
        if (rc < 0) return rc;
        for (size_t t = 0; t < m; t++) st[t] = (int8_t)valid[t];
      } else {  // no engine linked (the CPU test double): the same header's host build
        parallel_for(m, 8, [&](size_t t) {
          st[t] = tmv::secp::secp256k1_verify_msg(&pk[33 * t], 33, msg.data() + off[t], off[t + 1] - off[t],
                                                  &sig[64 * t], 64) ? 1 : 0;
        });
      }
    }
    for (size_t t = 0; t < m; t++)
      if (st[t] == 1) (ents[t].ext ? ext_ok : vote_ok)[ents[t].v] = 1;
  }

  int bad = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t failed = 0;
    if (results[i] == TMV_VOTE_OK) {
      if (!vote_ok[i]) failed = 1;
      else if (!ext_ok[i]) failed = 2;
      if (failed) results[i] = TMV_VOTE_ERR_INVALID_SIGNATURE;
    }
    if (failed_sig) failed_sig[i] = failed;
    bad += results[i] != TMV_VOTE_OK;
  }
  return bad;
}

}  // extern "C"
