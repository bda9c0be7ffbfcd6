// C-ABI of the validator-set arithmetic (valset_update.h): one
// UpdateWithChangeSet, NewValidatorSet, the per-block proposer rotation of
// State.Update, and ValidatorSet.Hash on the host for the sets the device
// call does not take.  No engine dependency: the CPU test builds link this
// file alone.
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "ripemd160.h"
#include "tm_light.h"
#include "valset_update.h"

namespace {

void put_text(char *err, size_t cap, const std::string &s) {
  if (!err || cap == 0) return;
  const size_t n = std::min(s.size(), cap - 1);
  std::memcpy(err, s.data(), n);
  err[n] = 0;
}

tmh::KeyType kind_of(uint8_t k) {
  return k == TMV_KIND_ED25519 ? tmh::KeyType::Ed25519 : k == TMV_KIND_SR25519 ? tmh::KeyType::Sr25519
       : k == TMV_KIND_SECP256K1 ? tmh::KeyType::Secp256k1 : tmh::KeyType::Other;
}
uint8_t kind_to(tmh::KeyType k) {
  return k == tmh::KeyType::Ed25519 ? TMV_KIND_ED25519 : k == tmh::KeyType::Sr25519 ? TMV_KIND_SR25519
       : k == tmh::KeyType::Secp256k1 ? TMV_KIND_SECP256K1 : TMV_KIND_OTHER;
}

tmh::Validator validator_of(const tmv_validator &v) {
  tmh::Validator o;
  o.address = tmh::ByteView(v.address, v.address_len);
  o.pub_key = tmh::PubKey{kind_of(v.key_kind), tmh::ByteView(v.pub_key, v.pub_key_len)};
  o.voting_power = v.voting_power;
  o.proposer_priority = v.proposer_priority;
  return o;
}

tmv_validator validator_to(const tmh::Validator &v) {
  tmv_validator o;
  o.address = v.address.data();
  o.address_len = (uint32_t)v.address.size();
  o.pub_key = v.pub_key.bytes.data();
  o.pub_key_len = (uint32_t)v.pub_key.bytes.size();
  o.key_kind = kind_to(v.pub_key.type);
  o.voting_power = v.voting_power;
  o.proposer_priority = v.proposer_priority;
  return o;
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

// The changes as NewValidator makes them: the address derived from the key
// into addr_scratch + 20 * i.
std::vector<tmh::Validator> changes_of(const tmv_validator_update *changes, uint32_t n, uint8_t *addr_scratch) {
  std::vector<tmh::Validator> out(n);
  for (uint32_t i = 0; i < n; i++) {
    const tmv_validator_update &c = changes[i];
    uint8_t *addr = addr_scratch + 20ull * i;
    address_of(c.key_kind, c.pub_key, c.pub_key_len, addr);
    out[i].address = tmh::ByteView(addr, 20);
    out[i].pub_key = tmh::PubKey{kind_of(c.key_kind), tmh::ByteView(c.pub_key, c.pub_key_len)};
    out[i].voting_power = c.power;
  }
  return out;
}

int finish(const tmh::ValsetResult &r, const tmh::ValidatorSet &vs, tmv_validator *out, uint32_t *n_out, char *err,
           size_t err_cap) {
  put_text(err, err_cap, r.text);
  if (!r) return r.code;
  for (size_t i = 0; i < vs.validators.size(); i++) out[i] = validator_to(vs.validators[i]);
  *n_out = (uint32_t)vs.validators.size();
  return TMV_VALSET_OK;
}

}  // namespace

extern "C" {

int tmv_validator_set_update(const tmv_validator *vals, uint32_t n_vals, const tmv_validator_update *changes,
                             uint32_t n_changes, int allow_deletes, uint8_t *addr_scratch, tmv_validator *out,
                             uint32_t out_cap, uint32_t *n_out, char *err, size_t err_cap) {
  if ((n_vals && !vals) || (n_changes && (!changes || !addr_scratch)) || !out || !n_out ||
      (uint64_t)out_cap < (uint64_t)n_vals + n_changes)
    return TMV_ERR_ARG;
  tmh::ValidatorSet vs;
  vs.validators.reserve(n_vals);
  for (uint32_t i = 0; i < n_vals; i++) vs.validators.push_back(validator_of(vals[i]));
  const tmh::ValsetResult r = tmh::UpdateWithChangeSet(vs, changes_of(changes, n_changes, addr_scratch), allow_deletes != 0);
  return finish(r, vs, out, n_out, err, err_cap);
}

int tmv_validator_set_new(const tmv_validator_update *vals, uint32_t n_vals, uint8_t *addr_scratch, tmv_validator *out,
                          uint32_t out_cap, uint32_t *n_out, int32_t *proposer_index, char *err, size_t err_cap) {
  if ((n_vals && (!vals || !addr_scratch)) || !out || !n_out || !proposer_index || out_cap < n_vals) return TMV_ERR_ARG;
  tmh::ValidatorSet vs;
  const tmh::ValsetResult r = tmh::NewValidatorSet(vs, changes_of(vals, n_vals, addr_scratch));
  *proposer_index = r ? vs.proposer : -1;
  return finish(r, vs, out, n_out, err, err_cap);
}

int tmv_validator_set_rotate(tmv_validator *vals, uint32_t n_vals, int32_t times, uint32_t steps,
                             int32_t *proposer_out, char *err, size_t err_cap) {
  if ((n_vals && !vals) || (steps && !proposer_out)) return TMV_ERR_ARG;
  tmh::ValidatorSet vs;
  vs.validators.reserve(n_vals);
  for (uint32_t i = 0; i < n_vals; i++) vs.validators.push_back(validator_of(vals[i]));
  for (uint32_t s = 0; s < steps; s++) {
    const tmh::ValsetResult r = tmh::IncrementProposerPriority(vs, times);
    if (!r) {  // the caller's priorities stay as they were
      put_text(err, err_cap, r.text);
      return r.code;
    }
    proposer_out[s] = vs.proposer;
  }
  put_text(err, err_cap, "");
  for (uint32_t i = 0; i < n_vals; i++) vals[i].proposer_priority = vs.validators[i].proposer_priority;
  return TMV_VALSET_OK;
}

int tmv_validator_set_hash_host(const tmv_validator *vals, uint32_t n_vals, uint8_t out[32]) {
  if ((n_vals && !vals) || !out) return TMV_ERR_ARG;
  tmh::ValidatorSet vs;
  vs.validators.reserve(n_vals);
  for (uint32_t i = 0; i < n_vals; i++) vs.validators.push_back(validator_of(vals[i]));
  const tmh::Bytes h = tmh::ValidatorSetHashHost(vs);
  std::memcpy(out, h.data(), 32);
  return 0;
}

}  // extern "C"
