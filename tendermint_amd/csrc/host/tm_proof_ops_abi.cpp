// ABCI query proofs and tx proofs of the host layer (include/tmhost.h):
//   tmv_proof_ops_verify     ProofRuntime.Verify under merkle.DefaultProofRuntime()
//       (crypto/merkle/proof_op.go:35-69,114-130; ValueOp.Run, proof_value.go:
//       77-98), what the light client's ABCIQueryWithOptions checks against a
//       trusted header's AppHash (light/rpc/client.go:148-217)
//   tmv_tx_proofs_validate   TxProof.Validate (types/tx.go:286-301), what
//       Tx(hash, prove) checks against DataHash (light/rpc/client.go:525-543)
// Large calls hash on the device through tmv_merkle_value_ops /
// tmv_merkle_verify_proofs, weak references as in tm_merkle_abi.cpp: a build
// of this file without the engine loads all the same and computes on the host
// worker pool with the SHA-256 of tm_light.h -- the same verdicts and texts.
// The device only hashes: the sequencing of ProofOperators.Verify and every
// text are host code shared by both paths.  Only the public tmv_* C-ABI is
// used to reach the device (layering).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "merkle_plan.h"
#include "tm_host_internal.h"
#include "tm_light.h"
#include "tm_proof_common.h"

extern "C" int tmv_merkle_value_ops(tmv_ctx *ctx, uint32_t flags, uint32_t n_items, const uint8_t *value,
                                    const uint32_t *value_off, const uint32_t *op_off, const uint8_t *key,
                                    const uint32_t *key_off, const int64_t *total, const int64_t *index,
                                    const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                                    const uint8_t *root, uint8_t *value_digest, uint8_t *kv_hash_calc,
                                    uint8_t *leaf_ok, uint8_t *root_calc, uint8_t *root_nil, int8_t *status_out,
                                    int32_t *fail_op_out) __attribute__((weak));
extern "C" int tmv_merkle_verify_proofs(tmv_ctx *ctx, uint32_t flags, uint32_t n, const int64_t *total,
                                        const int64_t *index, const uint8_t *leaf_hash, const uint8_t *aunts,
                                        const uint32_t *aunt_off, const uint8_t *root, const uint8_t *data,
                                        const uint32_t *leaf_off, int8_t *status_out, uint8_t *leaf_hash_calc,
                                        uint8_t *root_calc, uint8_t *root_nil) __attribute__((weak));

namespace {

using tmh::Bytes;
using tmh_internal::parallel_for;
using tmh_proof::hex_upper;
using tmh_proof::put;
using tmh_proof::root_from_aunts;
using tmh_proof::validate_basic;

constexpr uint64_t kEngineMaxBytes = 1ull << 30;  // the engine calls' limits per call
constexpr uint64_t kEngineMaxItems = 1ull << 26;
constexpr uint64_t kEngineMaxAunts = 1ull << 28;

// Calls with fewer ops (tx proofs: items) than this compute on the host.
// 10,000: the smallest swept size from which the device path, staging
// included, was faster than this file's host path for every shape with values
// of at most 1 KiB (by 16 % or more); at 1,000 to 2,000 ops the two are within
// 17 % of each other, one way or the other.
// TMV_DEVICE_PROOF_OPS_MIN overrides (ops; read on every call: tests change it).
uint64_t device_proof_ops_min() {
  const char *e = std::getenv("TMV_DEVICE_PROOF_OPS_MIN");
  return e ? (uint64_t)std::strtoull(e, nullptr, 10) : 10000ull;
}

// The device path's second condition: the call's values and keys (tx proofs:
// the txs) average at most this many bytes per op.  Staging moves a value byte
// at about half the rate at which the host pool hashes it, so long values only
// lose there: with 64 KiB values the device path took twice the host's time at
// every swept size, with 1 KiB values and 20-byte keys, 1,044 bytes per op, it
// still won: the default is that shape, the largest measured to win (DESIGN.md
// section 19).
// For tx proofs the figure is borrowed: only 250-byte txs were measured.
// TMV_DEVICE_PROOF_OPS_MAX_BYTES overrides (bytes per op; read on every call).
// Whatever the average, an item stays on the host when its keys hold more than
// this many bytes per op (k_merkle_value_ops reads a key byte by byte on one
// lane, and keys come from an untrusted node with no bound on their size), or
// its value more than 64 times this (one lane's serial chain: 64 KiB took
// 3.6 ms): one such item would make a whole window wait for a single lane.
uint64_t device_bytes_per_op() {
  const char *e = std::getenv("TMV_DEVICE_PROOF_OPS_MAX_BYTES");
  return e ? (uint64_t)std::strtoull(e, nullptr, 10) : 1044ull;
}
// Ops (tx proofs: items) per engine call.  Measured: one call over 100,000
// one-op items of 1 KiB took 95.0 ms (the host 89.2), in windows 59.9 to
// 70.7 ms.  Supposed cause, not measured: the one call's staging vectors of
// tens of MiB are fresh pages every time, the windows' stay small and warm.
// The smallest shape gains nothing from it (100,000 items of 32 B: 52.5 ms in
// one call, 54.0 and 62.9 ms in windows, where k_merkle_value_ops' summed time
// goes from 0.195 to 0.71 ms); it stays ahead of the host there.
constexpr uint64_t kWindowOps = 16384;

std::string str_of(const tmv_bytes &b) { return std::string(reinterpret_cast<const char *>(b.p), b.len); }

bool equal(const tmv_bytes &a, const uint8_t *p, size_t n) {  // bytes.Equal: nil equals empty
  return a.len == n && (n == 0 || std::memcmp(a.p, p, n) == 0);
}

void sha256(const uint8_t *pre, size_t pre_n, const uint8_t *p, size_t n, uint8_t out[32]) {
  uint32_t w[8];
  tmh::Sha256Bytes(w, pre, pre_n, p, n);
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(w[i] >> (24 - 8 * b));
}

// What ValueOp.Run computes for one op: the KV leaf hash and the root from the
// given leaf hash (empty: nil).
struct OpHashes {
  uint8_t kv[32];
  Bytes root;
};

// encodeByteSlice (crypto/merkle/types.go): uvarint(len) || bytes
void encode_byte_slice(Bytes &out, const uint8_t *p, size_t n) {
  uint64_t v = n;
  while (v >= 0x80) {
    out.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  out.push_back((uint8_t)v);
  out.insert(out.end(), p, p + n);
}

void run_op_host(const tmv_value_op &op, const uint8_t *value, size_t value_len, OpHashes &o) {
  static const uint8_t zero = 0;
  uint8_t vhash[32];
  sha256(nullptr, 0, value, value_len, vhash);
  Bytes kvp;
  kvp.reserve(op.key.len + 40);
  encode_byte_slice(kvp, op.key.p, op.key.len);
  encode_byte_slice(kvp, vhash, 32);
  sha256(&zero, 1, kvp.data(), kvp.size(), o.kv);  // leafHash
  o.root = root_from_aunts(op.proof);
}

// The ops of an item that pass ValidateBasic have 32-byte leaf hashes and
// aunts: they fit the engine's layout whatever else is wrong with them.
struct Plan {
  std::string early;  // a text decided before any hashing (empty: none)
  bool hash = false;  // the item's ops are to be hashed
};

// ProofOperators.Verify (proof_op.go:39-69) over hashed ops: hs[j] is op j's
// OpHashes (unused for items that end before Run).
std::string sequence(const tmv_proof_ops_in &it, const OpHashes *hs) {
  uint32_t keys = it.n_keys;
  const uint8_t *arg = it.value ? it.value->p : nullptr;
  size_t arg_len = it.value ? it.value->len : 0;
  const bool have_arg = it.value != nullptr;
  for (uint32_t j = 0; j < it.n_ops; j++) {
    const tmv_value_op &op = it.ops[j];
    if (op.key.len != 0) {
      if (keys == 0)
        return "key path has insufficient # of parts: expected no more keys but got " + str_of(op.key);
      const tmv_bytes &last = it.keys[keys - 1];
      if (!equal(last, op.key.p, op.key.len))
        return "key mismatch on operation #" + std::to_string(j) + ": expected " + str_of(last) + " but got " +
               str_of(op.key);
      keys--;
    }
    if (!have_arg) return "expected 1 arg, got 0";
    if (std::memcmp(hs[j].kv, op.proof.leaf_hash.p, 32) != 0)
      return "leaf hash mismatch: want " + hex_upper(op.proof.leaf_hash.p, 32) + " got " + hex_upper(hs[j].kv, 32);
    arg = hs[j].root.data();
    arg_len = hs[j].root.size();
  }
  if (!equal(it.root, arg, arg_len))
    return "calculated root hash is invalid: expected " + hex_upper(it.root.p, it.root.len) + " but got " +
           hex_upper(arg, arg_len);
  if (keys != 0) return "keypath not consumed all";
  return "";
}

// ---- tx proofs
struct TxVerdict {
  bool verify_ok = false;
};

bool tx_regular(const tmv_tx_proof_in &it) {  // fits tmv_merkle_verify_proofs' fixed 32-byte layout
  if (it.proof.leaf_hash.len != 32 || it.root_hash.len != 32) return false;
  for (uint32_t a = 0; a < it.proof.n_aunts; a++)
    if (it.proof.aunts[a].len != 32) return false;
  return true;
}

// Proof.Verify(RootHash, Tx.Hash()) (proof.go:52-68) for total > 0, index >= 0
bool tx_verify_host(const tmv_tx_proof_in &it) {
  static const uint8_t zero = 0;
  uint8_t th[32], lh[32];
  sha256(nullptr, 0, it.data.p, it.data.len, th);
  sha256(&zero, 1, th, 32, lh);
  if (!equal(it.proof.leaf_hash, lh, 32)) return false;
  const Bytes root = root_from_aunts(it.proof);
  return equal(it.root_hash, root.data(), root.size());  // a nil root equals an empty RootHash
}

}  // namespace

extern "C" {

int tmv_proof_ops_verify(tmv_ctx *ctx, const tmv_proof_ops_in *items, uint32_t n, int32_t *results, char *errs,
                         size_t err_stride) {
  if (n == 0) return 0;
  if (!items || !results) return TMV_ERR_ARG;
  for (uint32_t i = 0; i < n; i++) {
    const tmv_proof_ops_in &it = items[i];
    if ((it.n_ops && !it.ops) || (it.n_keys && !it.keys)) return TMV_ERR_ARG;
    for (uint32_t j = 0; j < it.n_ops; j++)
      if (it.ops[j].proof.n_aunts && !it.ops[j].proof.aunts) return TMV_ERR_ARG;
    if (it.n_ops == 0 && !it.value) return TMV_ERR_ARG;  // the reference indexes args[0] of nil and panics
  }
  // 1. every op's ValidateBasic, before anything else; which items hash at all
  std::vector<Plan> plan(n);
  std::vector<uint32_t> first(n + 1, 0);  // item i's ops in the flat arrays below
  parallel_for(n, 64, [&](size_t i) {
    const tmv_proof_ops_in &it = items[i];
    for (uint32_t j = 0; j < it.n_ops; j++) {
      const std::string e = validate_basic(it.ops[j].proof);
      if (!e.empty()) {
        plan[i].early = "decoding proof: decoding a proof operator: " + e;
        return;
      }
    }
    plan[i].hash = it.n_ops != 0 && it.value != nullptr;
  });
  uint64_t n_hash_ops = 0;
  std::vector<uint32_t> hashed;
  for (uint32_t i = 0; i < n; i++) {
    first[i + 1] = first[i];
    if (plan[i].hash) {
      hashed.push_back(i);
      first[i + 1] += items[i].n_ops;
      n_hash_ops += items[i].n_ops;
      if (n_hash_ops > 0xffffffffull) return TMV_ERR_ARG;
    }
  }
  std::vector<OpHashes> hs((size_t)n_hash_ops);
  // 2. the hashes: the device for large calls, the host pool otherwise
  std::vector<uint32_t> dev, host;
  const uint64_t per_op = std::min<uint64_t>(device_bytes_per_op(), 1ull << 24);  // products below stay in 64 bits
  uint64_t hashed_bytes = 0;  // values and keys
  for (uint32_t i : hashed) {
    hashed_bytes += items[i].value->len;
    for (uint32_t j = 0; j < items[i].n_ops; j++) hashed_bytes += items[i].ops[j].key.len;
  }
  const bool device = tmv_merkle_value_ops && ctx && n_hash_ops >= device_proof_ops_min() &&
                      hashed_bytes <= per_op * n_hash_ops;
  for (uint32_t i : hashed) {
    uint64_t kb = 0, na = 0;
    for (uint32_t j = 0; j < items[i].n_ops; j++) {
      kb += items[i].ops[j].key.len;
      na += items[i].ops[j].proof.n_aunts;
    }
    const bool fits = items[i].value->len <= kEngineMaxBytes && kb <= kEngineMaxBytes && na <= kEngineMaxAunts &&
                      items[i].n_ops <= kEngineMaxItems;
    const bool one_lane_ok = kb <= per_op * items[i].n_ops && items[i].value->len <= 64 * per_op;
    (device && fits && one_lane_ok ? dev : host).push_back(i);
  }
  parallel_for(host.size(), 1, [&](size_t k) {
    const tmv_proof_ops_in &it = items[host[k]];
    OpHashes *o = hs.data() + first[host[k]];
    const uint8_t *arg = it.value->p;
    size_t arg_len = it.value->len;
    for (uint32_t j = 0; j < it.n_ops; j++) {
      run_op_host(it.ops[j], arg, arg_len, o[j]);
      arg = o[j].root.data();
      arg_len = o[j].root.size();
    }
  });
  for (size_t lo = 0; lo < dev.size();) {  // windows within the engine's limits
    size_t hi = lo;
    uint64_t vb = 0, kb = 0, na = 0, no = 0;
    while (hi < dev.size() && hi - lo < kEngineMaxItems) {
      const tmv_proof_ops_in &it = items[dev[hi]];
      uint64_t k1 = 0, a1 = 0;
      for (uint32_t j = 0; j < it.n_ops; j++) {
        k1 += it.ops[j].key.len;
        a1 += it.ops[j].proof.n_aunts;
      }
      if (vb + it.value->len > kEngineMaxBytes || kb + k1 > kEngineMaxBytes || na + a1 > kEngineMaxAunts ||
          no + it.n_ops > kEngineMaxItems || (hi > lo && no + it.n_ops > kWindowOps))
        break;
      vb += it.value->len;
      kb += k1;
      na += a1;
      no += it.n_ops;
      hi++;
    }
    const uint32_t m = (uint32_t)(hi - lo), n_ops = (uint32_t)no;  // m >= 1: every item of dev fits alone
    std::vector<uint32_t> voff(m + 1, 0), ooff(m + 1, 0), koff(n_ops + 1, 0), aoff(n_ops + 1, 0);
    std::vector<int64_t> total(n_ops), index(n_ops);
    std::vector<uint8_t> value(vb), key(kb), lh(32ull * n_ops), aunts(32 * na), root(32ull * m, 0);
    for (uint32_t k = 0; k < m; k++) {
      const tmv_proof_ops_in &it = items[dev[lo + k]];
      voff[k + 1] = voff[k] + it.value->len;
      ooff[k + 1] = ooff[k] + it.n_ops;
      for (uint32_t j = 0; j < it.n_ops; j++) {
        const uint32_t o = ooff[k] + j;
        koff[o + 1] = koff[o] + it.ops[j].key.len;
        aoff[o + 1] = aoff[o] + it.ops[j].proof.n_aunts;
        total[o] = it.ops[j].proof.total;
        index[o] = it.ops[j].proof.index;
      }
    }
    parallel_for(m, 16, [&](size_t k) {
      const tmv_proof_ops_in &it = items[dev[lo + k]];
      if (it.value->len) std::memcpy(value.data() + voff[k], it.value->p, it.value->len);
      if (it.root.len == 32) std::memcpy(root.data() + 32ull * k, it.root.p, 32);  // other sizes: compared below
      for (uint32_t j = 0; j < it.n_ops; j++) {
        const uint32_t o = ooff[k] + j;
        const tmv_value_op &op = it.ops[j];
        if (op.key.len) std::memcpy(key.data() + koff[o], op.key.p, op.key.len);
        std::memcpy(lh.data() + 32ull * o, op.proof.leaf_hash.p, 32);
        for (uint32_t a = 0; a < op.proof.n_aunts; a++)
          std::memcpy(aunts.data() + 32ull * (aoff[o] + a), op.proof.aunts[a].p, 32);
      }
    });
    std::vector<uint8_t> kv(32ull * n_ops), rc(32ull * n_ops), nil(n_ops);
    const int rcode = tmv_merkle_value_ops(ctx, 0, m, vb ? value.data() : nullptr, voff.data(), ooff.data(),
                                           kb ? key.data() : nullptr, koff.data(), total.data(), index.data(),
                                           lh.data(), na ? aunts.data() : nullptr, aoff.data(), root.data(), nullptr,
                                           kv.data(), nullptr, rc.data(), nil.data(), nullptr, nullptr);
    if (rcode < 0) return rcode;
    for (uint32_t k = 0; k < m; k++) {
      OpHashes *o = hs.data() + first[dev[lo + k]];
      for (uint32_t j = 0; j < items[dev[lo + k]].n_ops; j++) {
        const uint32_t q = ooff[k] + j;
        std::memcpy(o[j].kv, kv.data() + 32ull * q, 32);
        if (!nil[q]) o[j].root.assign(rc.begin() + 32ull * q, rc.begin() + 32ull * q + 32);
      }
    }
    lo = hi;
  }
  // 3. the reference's sequence of tests and texts, the same for both paths
  std::vector<std::string> text(n);
  parallel_for(n, 64, [&](size_t i) {
    text[i] = !plan[i].early.empty() ? plan[i].early : sequence(items[i], hs.data() + first[i]);
  });
  int failed = 0;
  for (uint32_t i = 0; i < n; i++) {
    results[i] = text[i].empty() ? 0 : 1;
    put(errs, err_stride, i, text[i]);
    failed += results[i];
  }
  return failed;
}

int tmv_tx_proofs_validate(tmv_ctx *ctx, const tmv_tx_proof_in *items, uint32_t n, int32_t *results, char *errs,
                           size_t err_stride) {
  if (n == 0) return 0;
  if (!items || !results) return TMV_ERR_ARG;
  std::vector<const char *> text(n, nullptr);
  std::vector<uint32_t> dev, host;
  for (uint32_t i = 0; i < n; i++) {
    const tmv_tx_proof_in &it = items[i];
    if (it.proof.n_aunts && !it.proof.aunts) return TMV_ERR_ARG;
    if (!equal(it.data_hash, it.root_hash.p, it.root_hash.len)) text[i] = "proof matches different data hash";
    else if (it.proof.index < 0) text[i] = "proof index cannot be negative";
    else if (it.proof.total <= 0) text[i] = "proof total must be positive";
    else (tx_regular(it) && it.data.len <= kEngineMaxBytes && it.proof.n_aunts <= kEngineMaxAunts ? dev : host).push_back(i);
  }
  uint64_t tx_bytes = 0;
  for (uint32_t i : dev) tx_bytes += items[i].data.len;
  if (!tmv_merkle_verify_proofs || !ctx || dev.size() < device_proof_ops_min() ||
      tx_bytes > std::min<uint64_t>(device_bytes_per_op(), 1ull << 24) * dev.size()) {
    host.insert(host.end(), dev.begin(), dev.end());
    dev.clear();
  }
  std::vector<uint8_t> ok(n, 0);
  parallel_for(host.size(), 4, [&](size_t k) { ok[host[k]] = tx_verify_host(items[host[k]]) ? 1 : 0; });
  for (size_t lo = 0; lo < dev.size();) {
    size_t hi = lo;
    uint64_t sz = 0, na = 0;
    while (hi < dev.size() && hi - lo < kWindowOps && sz + items[dev[hi]].data.len <= kEngineMaxBytes &&
           na + items[dev[hi]].proof.n_aunts <= kEngineMaxAunts) {
      sz += items[dev[hi]].data.len;
      na += items[dev[hi]].proof.n_aunts;
      hi++;
    }
    const uint32_t m = (uint32_t)(hi - lo);  // >= 1: every item of dev fits alone
    std::vector<int64_t> total(m), index(m);
    std::vector<uint8_t> lh(32ull * m), root(32ull * m), aunts(32 * na), data(sz);
    std::vector<uint32_t> aoff(m + 1, 0), loff(m + 1, 0);
    for (uint32_t k = 0; k < m; k++) {
      const tmv_tx_proof_in &it = items[dev[lo + k]];
      total[k] = it.proof.total;
      index[k] = it.proof.index;
      aoff[k + 1] = aoff[k] + it.proof.n_aunts;
      loff[k + 1] = loff[k] + it.data.len;
    }
    parallel_for(m, 16, [&](size_t k) {
      const tmv_tx_proof_in &it = items[dev[lo + k]];
      std::memcpy(lh.data() + 32ull * k, it.proof.leaf_hash.p, 32);
      std::memcpy(root.data() + 32ull * k, it.root_hash.p, 32);
      for (uint32_t a = 0; a < it.proof.n_aunts; a++)
        std::memcpy(aunts.data() + 32ull * (aoff[k] + a), it.proof.aunts[a].p, 32);
      if (it.data.len) std::memcpy(data.data() + loff[k], it.data.p, it.data.len);
    });
    std::vector<int8_t> status(m);
    const int rc = tmv_merkle_verify_proofs(ctx, TMV_MERKLE_PREHASH, m, total.data(), index.data(), lh.data(),
                                            na ? aunts.data() : nullptr, aoff.data(), root.data(),
                                            sz ? data.data() : nullptr, loff.data(), status.data(), nullptr, nullptr,
                                            nullptr);
    if (rc < 0) return rc;
    for (uint32_t k = 0; k < m; k++) ok[dev[lo + k]] = status[k] == 0;
    lo = hi;
  }
  int failed = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!text[i] && !ok[i]) text[i] = "proof is not internally consistent";
    results[i] = text[i] ? 1 : 0;
    put(errs, err_stride, i, text[i] ? text[i] : "");
    failed += results[i];
  }
  return failed;
}

}  // extern "C"
