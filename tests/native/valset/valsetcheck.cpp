// C entry points over csrc/host/valset_update.h for tests/test_valset_update.py:
// the change set with the addresses given (the reference's own tests name
// their validators by address, with no key), beside the product's C-ABI
// (csrc/host/tm_valset_abi.cpp), which derives them from the keys.
#include <cstring>

#include "../../../include/tmhost.h"
#include "host/valset_update.h"

namespace {

tmh::Validator of(const tmv_validator &v) {
  tmh::Validator o;
  o.address = tmh::ByteView(v.address, v.address_len);
  o.pub_key = tmh::PubKey{tmh::KeyType::Ed25519, tmh::ByteView(v.pub_key, v.pub_key_len)};
  o.voting_power = v.voting_power;
  o.proposer_priority = v.proposer_priority;
  return o;
}

}  // namespace

extern "C" {

// UpdateWithChangeSet (is_new == 0) or NewValidatorSet (is_new != 0, vals
// ignored) with `changes` as validators: address, power.  out as
// tmv_validator_set_update; *proposer_index = the proposer after
// NewValidatorSet, else -1.  Returns the TMV_VALSET_* code.
int vs_update_by_address(const tmv_validator *vals, uint32_t n_vals, const tmv_validator *changes, uint32_t n_changes,
                         int is_new, tmv_validator *out, uint32_t *n_out, int32_t *proposer_index, char *err,
                         size_t err_cap) {
  tmh::ValidatorSet vs;
  std::vector<tmh::Validator> ch;
  for (uint32_t i = 0; i < n_changes; i++) ch.push_back(of(changes[i]));
  tmh::ValsetResult r;
  if (is_new) {
    r = tmh::NewValidatorSet(vs, ch);
  } else {
    for (uint32_t i = 0; i < n_vals; i++) vs.validators.push_back(of(vals[i]));
    r = tmh::UpdateWithChangeSet(vs, ch);
  }
  if (err && err_cap) {
    std::strncpy(err, r.text.c_str(), err_cap - 1);
    err[err_cap - 1] = 0;
  }
  *proposer_index = r && is_new ? vs.proposer : -1;
  if (!r) return r.code;
  for (size_t i = 0; i < vs.validators.size(); i++) {
    const tmh::Validator &v = vs.validators[i];
    out[i] = tmv_validator{v.address.data(), (uint32_t)v.address.size(), v.pub_key.bytes.data(),
                           (uint32_t)v.pub_key.bytes.size(), TMV_KIND_ED25519, v.voting_power, v.proposer_priority};
  }
  *n_out = (uint32_t)vs.validators.size();
  return 0;
}

}  // extern "C"
