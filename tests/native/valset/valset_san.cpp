// The validator-set arithmetic (csrc/host/valset_update.h) and its C-ABI
// (csrc/host/tm_valset_abi.cpp) under ASan + UBSan, as a stand-alone program
// (make -C tests/native/valset san; run by tests/test_valset_update.py):
//   * every script of tests/golden/validator_updates.json (the language is
//     described in tests/golden/make_validator_updates_golden.py) through the
//     header's functions, each expectation checked;
//   * the C-ABI over the edge inputs of the CPU tests: priorities within a few
//     units of +-2^63 (clipping, the wrapped max - min, a wrapped ratio), a
//     negative sum that n does not divide, negative priorities under a rescale,
//     total power at MaxTotalVotingPower and one above, sets of one and two,
//     everyone removed and one added, empty sets, times <= 0 -- with the output
//     arrays allocated at exactly the size the header asks for.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "host/valset_update.h"

namespace {

long checks = 0, wrong = 0;

void expect(bool ok, const std::string &what) {
  checks++;
  if (!ok) {
    wrong++;
    std::printf("wrong: %s\n", what.c_str());
  }
}

// every "<key>": "<text>" of the file, in order
std::vector<std::string> values_of(const std::string &text, const std::string &key) {
  std::vector<std::string> out;
  const std::string pat = "\"" + key + "\": \"";
  for (size_t at = text.find(pat); at != std::string::npos; at = text.find(pat, at + 1)) {
    const size_t lo = at + pat.size(), hi = text.find('"', lo);
    out.push_back(text.substr(lo, hi - lo));
  }
  return out;
}

std::vector<std::string> split(const std::string &s, const std::string &sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (size_t hit; (hit = s.find(sep, at)) != std::string::npos; at = hit + sep.size()) out.push_back(s.substr(at, hit - at));
  out.push_back(s.substr(at));
  return out;
}

// addresses live as long as the program: the validators hold views of them
std::map<std::string, tmh::Bytes> addresses;

tmh::ByteView address(const std::string &tok) {
  auto it = addresses.find(tok);
  if (it == addresses.end()) {
    tmh::Bytes b;
    if (tok.rfind("0x", 0) == 0)
      for (size_t i = 2; i + 1 < tok.size(); i += 2) b.push_back((uint8_t)std::stoi(tok.substr(i, 2), nullptr, 16));
    else
      b.assign(tok.begin(), tok.end());
    it = addresses.emplace(tok, std::move(b)).first;
  }
  return tmh::ByteView(it->second);
}

tmh::Validator validator(const std::string &tok) {
  const auto f = split(tok, ":");
  tmh::Validator v;
  v.address = address(f[0]);
  v.voting_power = std::stoll(f[1]);
  v.proposer_priority = f.size() > 2 ? std::stoll(f[2]) : 0;
  return v;
}

std::vector<tmh::Validator> validators(const std::vector<std::string> &args, size_t from = 0) {
  std::vector<tmh::Validator> out;
  for (size_t i = from; i < args.size(); i++)
    if (!args[i].empty()) out.push_back(validator(args[i]));
  return out;
}

bool same_members(const tmh::ValidatorSet &a, const std::vector<tmh::Validator> &b, bool priorities) {
  if (a.validators.size() != b.size()) return false;
  for (size_t i = 0; i < b.size(); i++)
    if (a.validators[i].address != b[i].address || a.validators[i].voting_power != b[i].voting_power ||
        (priorities && a.validators[i].proposer_priority != b[i].proposer_priority))
      return false;
  return true;
}

void verify(const tmh::ValidatorSet &vs, const std::string &what) {
  int64_t tvp = 0, tpp = 0;
  expect((bool)tmh::CheckedTotalVotingPower(vs.validators, &tvp), what + ": total power");
  for (const auto &v : vs.validators) tpp = tmh::SafeAddClip(tpp, v.proposer_priority);
  const int64_t n = (int64_t)vs.validators.size();
  expect(tpp < n && tpp > -n, what + ": not centred");
  expect(tmh::MaxMinPriorityDiff(vs.validators) <= tmh::kPriorityWindowSizeFactor * tvp, what + ": not scaled");
}

void run_script(const std::string &script, const std::string &name) {
  tmh::ValidatorSet vs;
  for (const std::string &step : split(script, "; ")) {
    const auto a = split(step, " ");
    const std::string &op = a[0], what = name + ": " + step.substr(0, 60);
    if (op == "new") {
      expect((bool)tmh::NewValidatorSet(vs, validators(a, 1)), what);
    } else if (op == "raw") {
      vs = tmh::ValidatorSet();
      vs.validators = validators(a, 1);
    } else if (op == "inc") {
      expect((bool)tmh::IncrementProposerPriority(vs, (int32_t)std::stol(a[1])), what);
    } else if (op == "upd") {
      expect((bool)tmh::UpdateWithChangeSet(vs, validators(a, 1)), what);
    } else if (op == "upd!") {
      const tmh::ValidatorSet before = vs;
      const tmh::ValsetResult r = tmh::UpdateWithChangeSet(vs, validators(a, 1));
      expect(r.code == tmh::kValsetError && !r.text.empty(), what + ": no error");
      expect(same_members(vs, before.validators, true), what + ": the set changed");
    } else if (op == "vals") {
      expect(same_members(vs, validators(a, 1), false), what);
    } else if (op == "prios") {
      bool ok = a.size() - 1 == vs.validators.size();
      for (size_t i = 1; ok && i < a.size(); i++) ok = vs.validators[i - 1].proposer_priority == std::stoll(a[i]);
      expect(ok, what);
    } else if (op == "prop") {
      const tmh::Validator *p = vs.GetProposer();
      expect(p && p->address == address(a[1]), what);
    } else if (op == "seq" || op == "count") {
      std::map<std::string, long> count;
      bool ok = true;
      for (long i = 0; i < std::stol(a[1]); i++) {
        const tmh::Validator *p = vs.GetProposer();
        if (op == "seq") ok = ok && p && p->address == address(a[2 + (size_t)i]);
        for (const auto &kv : addresses)
          if (p && p->address == tmh::ByteView(kv.second)) count[kv.first]++;
        ok = ok && (bool)tmh::IncrementProposerPriority(vs, 1);
      }
      if (op == "count")
        for (size_t i = 2; i < a.size(); i++) {
          const auto f = split(a[i], ":");
          ok = ok && count[f[0]] == std::stol(f[1]);
        }
      expect(ok, what);
    } else if (op == "verify") {
      verify(vs, what);
    } else if (op == "added") {
      int64_t lowest = INT64_MAX;
      for (const auto &v : vs.validators) lowest = std::min(lowest, v.proposer_priority);
      bool ok = true;
      for (size_t i = 1; i < a.size(); i++) {
        auto [idx, v] = vs.GetByAddress(address(a[i]));
        ok = ok && v && v->proposer_priority == lowest;
      }
      expect(ok, what);
    } else {
      expect(false, what + ": unknown step");
    }
  }
}

// ---- the C-ABI over edge inputs, every buffer on the heap at its exact size
struct Keys {
  std::vector<std::vector<uint8_t>> k;
  const uint8_t *make(uint8_t kind, uint32_t seed) {
    std::vector<uint8_t> b(kind == TMV_KIND_SECP256K1 ? 33 : 32);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)(seed * 131 + i * 7 + kind);
    k.push_back(std::move(b));
    return k.back().data();
  }
};

void abi_edges() {
  const int64_t kMax = tmh::kMaxTotalVotingPower;
  const std::vector<std::vector<int64_t>> prios = {
      {0}, {INT64_MIN}, {0, 0}, {11, 11, 11, 11, 11}, {INT64_MAX - 2, INT64_MIN + 3, INT64_MAX, INT64_MIN},
      {INT64_MAX, -1}, {INT64_MAX, 0}, {INT64_MAX - 1, INT64_MAX - 5, INT64_MAX}, {INT64_MIN + 1, INT64_MIN + 5, INT64_MIN},
      {-5, -3, 1}, {-7, 9, -1, 3}, {-25, 10, -11}, {37, -31, 48}};
  const std::vector<std::vector<int64_t>> powers = {{7}, {5, 5}, {3, 9}, {10, 1}, {1, 1, 1, 1}, {17, 1, 2}, {1000},
                                                    {kMax - 1, 1}, {kMax, 1}, {1LL << 40}};
  Keys keys;
  uint32_t seed = 0;
  for (const auto &pr : prios)
    for (const auto &pw : powers) {
      const uint32_t n = (uint32_t)pr.size();
      // the set: its own addresses (derived through a NewValidatorSet call, so they match the keys)
      std::vector<tmv_validator_update> members(n);
      for (uint32_t i = 0; i < n; i++) {
        const uint8_t kind = (uint8_t)((seed + i) % 3 == 2 ? TMV_KIND_SECP256K1 : (seed + i) % 3);
        members[i] = tmv_validator_update{kind, keys.make(kind, ++seed), kind == TMV_KIND_SECP256K1 ? 33u : 32u, 1};
      }
      uint8_t *scratch0 = (uint8_t *)std::malloc(20 * n);
      tmv_validator *set = (tmv_validator *)std::malloc(sizeof(tmv_validator) * n);
      uint32_t n_set = 0;
      int32_t prop = -2;
      char err[256];
      int rc = tmv_validator_set_new(members.data(), n, scratch0, set, n, &n_set, &prop, err, sizeof err);
      expect(rc == TMV_VALSET_OK && n_set == n && prop >= 0 && prop < (int32_t)n, "abi: new");
      for (uint32_t i = 0; i < n; i++) {
        set[i].voting_power = pw[i % pw.size()];
        set[i].proposer_priority = pr[i];
      }
      // rotations
      for (int32_t times : {1, 3, 0, -1})
        for (uint32_t steps : {0u, 1u, 4u}) {
          std::vector<tmv_validator> copy(set, set + n);
          int32_t *props = (int32_t *)std::malloc(sizeof(int32_t) * (steps ? steps : 1));
          rc = tmv_validator_set_rotate(copy.data(), n, times, steps, steps ? props : nullptr, err, sizeof err);
          checks++;
          if (rc == TMV_VALSET_OK)
            for (uint32_t s = 0; s < steps; s++) expect(props[s] >= 0 && props[s] < (int32_t)n, "abi: proposer index");
          else
            expect(rc == TMV_VALSET_PANIC && err[0] != 0, "abi: rotate code");
          std::free(props);
        }
      // change sets: a power change, the last one out and one in, everyone out and one in, everyone out
      for (int shape = 0; shape < 5; shape++) {
        std::vector<tmv_validator_update> ch;
        auto member = [&](uint32_t i, int64_t power) {
          ch.push_back(tmv_validator_update{set[i].key_kind, set[i].pub_key, set[i].pub_key_len, power});
        };
        auto fresh = [&](int64_t power) {
          ch.push_back(tmv_validator_update{TMV_KIND_ED25519, keys.make(TMV_KIND_ED25519, ++seed), 32, power});
        };
        if (shape == 0) member(0, set[0].voting_power % 1000 + 1);
        if (shape == 1) { member(n - 1, 0); fresh(3); }
        if (shape == 2) { for (uint32_t i = 0; i < n; i++) member(i, 0); fresh(4); }
        if (shape == 3) for (uint32_t i = 0; i < n; i++) member(i, 0);
        if (shape == 4) { fresh(kMax); fresh(-1); }
        const uint32_t nc = (uint32_t)ch.size();
        uint8_t *scratch = (uint8_t *)std::malloc(20 * nc);
        tmv_validator *out = (tmv_validator *)std::malloc(sizeof(tmv_validator) * (n + nc));
        uint32_t n_out = 0;
        for (int allow : {1, 0}) {
          rc = tmv_validator_set_update(set, n, ch.data(), nc, allow, scratch, out, n + nc, &n_out, err, sizeof err);
          expect(rc == TMV_VALSET_OK || ((rc == TMV_VALSET_ERROR || rc == TMV_VALSET_PANIC) && err[0] != 0), "abi: update code");
          if (rc == TMV_VALSET_OK) {
            expect(n_out >= 1 && n_out <= n + nc, "abi: size of the new set");
            uint8_t h[32];
            expect(tmv_validator_set_hash_host(out, n_out, h) == 0, "abi: hash");
            for (uint32_t i = 0; i + 1 < n_out; i++)
              expect(out[i].voting_power >= out[i + 1].voting_power, "abi: set order");
          }
        }
        std::free(out);
        std::free(scratch);
      }
      std::free(set);
      std::free(scratch0);
    }
  // argument errors and the empty set
  char err[64];
  uint32_t n_out = 7;
  int32_t prop = 7;
  tmv_validator one;
  expect(tmv_validator_set_rotate(nullptr, 0, 1, 0, nullptr, err, sizeof err) == TMV_VALSET_OK, "abi: no steps on no set");
  expect(tmv_validator_set_rotate(nullptr, 0, 1, 1, &prop, err, sizeof err) == TMV_VALSET_PANIC &&
             std::string(err) == "empty validator set", "abi: empty set");
  expect(tmv_validator_set_rotate(nullptr, 2, 1, 1, &prop, err, sizeof err) == TMV_ERR_ARG, "abi: null set");
  expect(tmv_validator_set_new(nullptr, 0, nullptr, &one, 0, &n_out, &prop, err, sizeof err) == TMV_VALSET_OK && n_out == 0 &&
             prop == -1, "abi: new empty set");
  expect(tmv_validator_set_update(nullptr, 0, nullptr, 0, 1, nullptr, &one, 0, &n_out, nullptr, 0) == TMV_VALSET_OK,
         "abi: nothing to do");
  expect(tmv_validator_set_update(nullptr, 0, nullptr, 1, 1, nullptr, &one, 1, &n_out, err, sizeof err) == TMV_ERR_ARG,
         "abi: null changes");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: valset_san validator_updates.json\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  std::stringstream ss;
  ss << f.rdbuf();
  const auto scripts = values_of(ss.str(), "script"), names = values_of(ss.str(), "name");
  if (scripts.empty() || scripts.size() != names.size()) {
    std::printf("no cases in %s\n", argv[1]);
    return 2;
  }
  for (size_t k = 0; k < scripts.size(); k++) run_script(scripts[k], names[k]);
  abi_edges();
  std::printf("%zu scripts\n%ld checks\n%ld wrong\n", scripts.size(), checks, wrong);
  return wrong ? 1 : 0;
}
