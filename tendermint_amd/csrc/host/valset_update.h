// Validator-set arithmetic of the reference, in C++: what State.Update
// (internal/state/execution.go:527-595) does to NextValidators once per block.
// Pure functions over tmh::ValidatorSet, no engine dependency (header-only,
// like tm_types.h), so the CPU test builds link them.
//
//   types/validator_set.go:70-80     NewValidatorSet
//   types/validator_set.go:116-138   IncrementProposerPriority(times)
//   types/validator_set.go:143-164   RescalePriorities
//   types/validator_set.go:166-234   incrementProposerPriority,
//                                    computeAvgProposerPriority,
//                                    computeMaxMinPriorityDiff,
//                                    shiftByAvgProposerPriority
//   types/validator_set.go:295-309   updateTotalVotingPower
//   types/validator_set.go:370-650   processChanges, verifyUpdates,
//                                    numNewValidators, computeNewPriorities,
//                                    applyUpdates, verifyRemovals,
//                                    applyRemovals, updateWithChangeSet
//   types/validator_set.go:870-908   safeAdd / safeSub / safeAddClip / safeSubClip
//
// Error texts are the reference's.  Where the reference panics the functions
// return kValsetPanic with the panic's text and leave the set as it was.
//
// The arithmetic that is easy to get wrong:
//   * the average priority is big.Int.Div -- Euclidean, the floor for the
//     positive divisor n -- over a sum that needs more than 64 bits;
//   * ProposerPriority /= ratio is Go's truncating int64 division;
//   * max - min of the priorities and diff + diffMax - 1 wrap as Go's int64
//     does (computed here in uint64_t, so nothing overflows a signed type);
//   * the increments clip (safeAddClip / safeSubClip) and never wrap.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "tm_types.h"

namespace tmh {

constexpr int64_t kMaxTotalVotingPower = INT64_MAX / 8;  // types/validator_set.go:25
constexpr int64_t kPriorityWindowSizeFactor = 2;         // types/validator_set.go:30

enum ValsetCode : int { kValsetOk = 0, kValsetError = 1, kValsetPanic = 2 };

struct ValsetResult {
  ValsetCode code = kValsetOk;
  std::string text;
  explicit operator bool() const { return code == kValsetOk; }
};
inline ValsetResult ValsetErr(std::string s) { return {kValsetError, std::move(s)}; }
inline ValsetResult ValsetPanic(std::string s) { return {kValsetPanic, std::move(s)}; }

// Go's int64 +, - and unary minus: two's complement, no trap.
inline int64_t WrapAdd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
inline int64_t WrapSub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
inline int64_t WrapNeg(int64_t a) { return (int64_t)((uint64_t)0 - (uint64_t)a); }
// Go's int64 /: truncates towards zero; MinInt64 / -1 is MinInt64.  b != 0.
inline int64_t GoDiv(int64_t a, int64_t b) { return b == -1 ? WrapNeg(a) : a / b; }

inline int64_t SafeAddClip(int64_t a, int64_t b) {
  if (b > 0 && a > INT64_MAX - b) return INT64_MAX;
  if (b < 0 && a < INT64_MIN - b) return INT64_MIN;
  return a + b;
}
inline int64_t SafeSubClip(int64_t a, int64_t b) {
  if (b > 0 && a < INT64_MIN + b) return INT64_MIN;
  if (b < 0 && a > INT64_MAX + b) return INT64_MAX;
  return a - b;
}

inline std::string ErrTotalVotingPowerOverflow() {
  return "total voting power of resulting valset exceeds max " + std::to_string(kMaxTotalVotingPower);
}

// fmt's %v of a []*Validator
inline std::string ValidatorListString(const std::vector<Validator> &l) {
  std::string s = "[";
  for (size_t i = 0; i < l.size(); i++) s += (i ? " " : "") + l[i].String();
  return s + "]";
}

// updateTotalVotingPower: the clipped sum, a panic above MaxTotalVotingPower.
inline ValsetResult CheckedTotalVotingPower(const std::vector<Validator> &vals, int64_t *total) {
  int64_t sum = 0;
  for (const Validator &v : vals) {
    sum = SafeAddClip(sum, v.voting_power);
    if (sum > kMaxTotalVotingPower)
      return ValsetPanic("Total voting power should be guarded to not exceed " + std::to_string(kMaxTotalVotingPower) +
                         "; got: " + std::to_string(sum));
  }
  *total = sum;
  return {};
}

// computeMaxMinPriorityDiff of a non-empty list.
inline int64_t MaxMinPriorityDiff(const std::vector<Validator> &vals) {
  int64_t mx = INT64_MIN, mn = INT64_MAX;
  for (const Validator &v : vals) {
    mn = std::min(mn, v.proposer_priority);
    mx = std::max(mx, v.proposer_priority);
  }
  const int64_t diff = WrapSub(mx, mn);
  return diff < 0 ? WrapNeg(diff) : diff;  // -MinInt64 stays MinInt64, as in Go
}

inline ValsetResult RescalePriorities(ValidatorSet &vs, int64_t diff_max) {
  if (vs.validators.empty()) return ValsetPanic("empty validator set");
  if (diff_max <= 0) return {};
  const int64_t diff = MaxMinPriorityDiff(vs.validators);
  if (diff > diff_max) {
    const int64_t ratio = GoDiv(WrapSub(WrapAdd(diff, diff_max), 1), diff_max);  // not 0: |diff + diffMax - 1| >= diffMax
    for (Validator &v : vs.validators) v.proposer_priority = GoDiv(v.proposer_priority, ratio);
  }
  return {};
}

// computeAvgProposerPriority: floor(sum / n) -- big.Int.Div is Euclidean.
inline int64_t AvgProposerPriority(const std::vector<Validator> &vals) {
  __int128 sum = 0;
  for (const Validator &v : vals) sum += v.proposer_priority;
  const __int128 n = (__int128)vals.size();
  __int128 q = sum / n;
  if (sum % n < 0) q -= 1;
  return (int64_t)q;  // between the smallest and the largest priority
}

inline ValsetResult ShiftByAvgProposerPriority(ValidatorSet &vs) {
  if (vs.validators.empty()) return ValsetPanic("empty validator set");
  const int64_t avg = AvgProposerPriority(vs.validators);
  for (Validator &v : vs.validators) v.proposer_priority = SafeSubClip(v.proposer_priority, avg);
  return {};
}

// incrementProposerPriority: one election.  The winner is GetProposer's
// choice with no proposer recorded (highest priority, ties to the smaller
// address); the reference panics on two equal addresses, which a set built by
// the functions here never holds.
inline void IncrementOnce(ValidatorSet &vs, int64_t total) {
  for (Validator &v : vs.validators) v.proposer_priority = SafeAddClip(v.proposer_priority, v.voting_power);
  vs.proposer = -1;
  const Validator *most = vs.GetProposer();
  vs.proposer = (int)(most - vs.validators.data());
  Validator &m = vs.validators[(size_t)vs.proposer];
  m.proposer_priority = SafeSubClip(m.proposer_priority, total);
}

// IncrementProposerPriority(times): rescale and centre once, then `times`
// elections; vs.proposer = the last winner.
inline ValsetResult IncrementProposerPriority(ValidatorSet &vs, int32_t times) {
  if (vs.validators.empty()) return ValsetPanic("empty validator set");
  if (times <= 0) return ValsetPanic("Cannot call IncrementProposerPriority with non-positive times");
  int64_t total = 0;
  if (ValsetResult r = CheckedTotalVotingPower(vs.validators, &total); !r) return r;
  RescalePriorities(vs, kPriorityWindowSizeFactor * total);  // neither fails on a non-empty set
  ShiftByAvgProposerPriority(vs);
  vs.total_voting_power = total;
  for (int32_t i = 0; i < times; i++) IncrementOnce(vs, total);
  return {};
}

namespace valset_detail {

inline bool AddressLess(const Validator &a, const Validator &b) { return a.address < b.address; }

// the set's validators by address, for the lookups of one change set:
// GetByAddress is a linear scan in the reference, and a change set of m
// entries over n validators would cost m * n here
struct ByAddress {
  std::vector<const Validator *> sorted;
  explicit ByAddress(const std::vector<Validator> &vals) {
    sorted.reserve(vals.size());
    for (const Validator &v : vals) sorted.push_back(&v);
    std::stable_sort(sorted.begin(), sorted.end(),
                     [](const Validator *a, const Validator *b) { return a->address < b->address; });
  }
  // the first validator in set order with this address, as GetByAddress
  const Validator *operator()(ByteView addr) const {
    auto it = std::lower_bound(sorted.begin(), sorted.end(), addr,
                               [](const Validator *a, ByteView k) { return a->address < k; });
    return it != sorted.end() && (*it)->address == addr ? *it : nullptr;
  }
};

}  // namespace valset_detail

// updateWithChangeSet.  `changes` hold address, key and power (the priority
// of an entry is ignored, as computeNewPriorities overwrites it).  On any
// result but kValsetOk the set is unchanged.  The validators of the new set
// are copies of the views in `vs` and `changes`: the bytes they point to must
// outlive it.  vs.proposer is left at -1: the reference keeps a pointer to the
// proposer's old copy, and every caller goes on to IncrementProposerPriority.
inline ValsetResult UpdateWithChangeSet(ValidatorSet &vs, const std::vector<Validator> &changes_in,
                                        bool allow_deletes = true) {
  using namespace valset_detail;
  if (changes_in.empty()) return {};

  // processChanges
  std::vector<Validator> changes = changes_in;
  std::stable_sort(changes.begin(), changes.end(), AddressLess);
  std::vector<Validator> updates, deletes;
  for (size_t i = 0; i < changes.size(); i++) {
    const Validator &c = changes[i];
    // prevAddr starts nil, and bytes.Equal(empty, nil) holds: an empty first address is a duplicate
    if (i == 0 ? c.address.empty() : c.address == changes[i - 1].address)
      return ValsetErr("duplicate entry " + c.String() + " in " + ValidatorListString(changes));
    if (c.voting_power < 0) return ValsetErr("voting power can't be negative: " + std::to_string(c.voting_power));
    if (c.voting_power > kMaxTotalVotingPower)
      return ValsetErr("to prevent clipping/overflow, voting power can't be higher than " +
                       std::to_string(kMaxTotalVotingPower) + ", got " + std::to_string(c.voting_power));
    (c.voting_power == 0 ? deletes : updates).push_back(c);
  }
  if (!allow_deletes && !deletes.empty())
    return ValsetErr("cannot process validators with voting power 0: " + ValidatorListString(deletes));

  const ByAddress find(vs.validators);
  // numNewValidators
  size_t n_new = 0;
  for (const Validator &u : updates) n_new += find(u.address) == nullptr;
  if (n_new == 0 && vs.validators.size() == deletes.size())
    return ValsetErr("applying the validator changes would result in empty set");

  // verifyRemovals
  int64_t removed = 0;
  for (const Validator &d : deletes) {
    const Validator *v = find(d.address);
    if (!v) return ValsetErr("failed to find validator " + HexUpper(d.address) + " to remove");
    removed = WrapAdd(removed, v->voting_power);
  }
  if (deletes.size() > vs.validators.size()) return ValsetPanic("more deletes than validators");

  // verifyUpdates: the deltas in ascending order, so that the decreases come first
  int64_t total = 0;
  if (ValsetResult r = CheckedTotalVotingPower(vs.validators, &total); !r) return r;
  std::vector<int64_t> delta;
  delta.reserve(updates.size());
  for (const Validator &u : updates) {
    const Validator *v = find(u.address);
    delta.push_back(v ? WrapSub(u.voting_power, v->voting_power) : u.voting_power);
  }
  std::sort(delta.begin(), delta.end());
  int64_t tvp = WrapSub(total, removed);
  for (int64_t d : delta) {
    tvp = WrapAdd(tvp, d);
    if (tvp > kMaxTotalVotingPower) return ValsetErr(ErrTotalVotingPowerOverflow());
  }
  tvp = WrapAdd(tvp, removed);  // tvpAfterUpdatesBeforeRemovals

  // computeNewPriorities
  for (Validator &u : updates) {
    const Validator *v = find(u.address);
    u.proposer_priority = v ? v->proposer_priority : WrapNeg(WrapAdd(tvp, tvp >> 3));
  }

  // applyUpdates, applyRemovals: one merge over both address-sorted lists
  std::vector<Validator> merged;
  merged.reserve(vs.validators.size() + updates.size());
  {
    size_t e = 0, u = 0;
    const auto &ex = find.sorted;
    while (e < ex.size() && u < updates.size()) {
      if (ex[e]->address < updates[u].address) {
        merged.push_back(*ex[e++]);
      } else {
        if (ex[e]->address == updates[u].address) e++;
        merged.push_back(updates[u++]);
      }
    }
    for (; e < ex.size(); e++) merged.push_back(*ex[e]);
    for (; u < updates.size(); u++) merged.push_back(updates[u]);
  }
  if (!deletes.empty()) {
    std::vector<Validator> kept;
    kept.reserve(merged.size() - deletes.size());
    size_t d = 0;
    for (const Validator &m : merged) {
      if (d < deletes.size() && m.address == deletes[d].address) d++;
      else kept.push_back(m);
    }
    merged.swap(kept);
  }

  ValidatorSet next;
  next.validators.swap(merged);
  if (ValsetResult r = CheckedTotalVotingPower(next.validators, &next.total_voting_power); !r) return r;
  if (ValsetResult r = RescalePriorities(next, kPriorityWindowSizeFactor * next.total_voting_power); !r) return r;
  if (ValsetResult r = ShiftByAvgProposerPriority(next); !r) return r;
  // ValidatorsByVotingPower: power descending, address ascending
  std::sort(next.validators.begin(), next.validators.end(), [](const Validator &a, const Validator &b) {
    return a.voting_power != b.voting_power ? a.voting_power > b.voting_power : a.address < b.address;
  });
  next.proposer = -1;
  vs = std::move(next);
  return {};
}

// NewValidatorSet: the change set over an empty set with deletes refused, then
// one IncrementProposerPriority(1) when the set is not empty.  The reference
// panics on an error of the change set.
inline ValsetResult NewValidatorSet(ValidatorSet &out, const std::vector<Validator> &valz) {
  ValidatorSet vs;
  if (ValsetResult r = UpdateWithChangeSet(vs, valz, false); !r)
    return r.code == kValsetError ? ValsetPanic("cannot create validator set: " + r.text) : r;
  if (!valz.empty())
    if (ValsetResult r = IncrementProposerPriority(vs, 1); !r) return r;
  out = std::move(vs);
  return {};
}

}  // namespace tmh
