"""Restatement of the reference's validator-set arithmetic
(types/validator_set.go:70-234, 362-650, 870-908) in Python's unbounded
integers, with Go's int64 behaviour written out where it matters: the checker
for tendermint_amd/csrc/host/valset_update.h.

A validator is a Val(address, power, priority, key, kind); a set is a list of
Val in set order.  The functions return new lists and raise ValsetError (the
reference returns an error) or ValsetPanic (it panics), with its text.
"""
import hashlib
from dataclasses import dataclass, replace

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_TOTAL_VOTING_POWER = I64_MAX // 8
PRIORITY_WINDOW_SIZE_FACTOR = 2
KIND_NAMES = {0: "Ed25519", 1: "Sr25519", 3: "Secp256k1"}


class ValsetError(Exception):
    pass


class ValsetPanic(Exception):
    pass


@dataclass(frozen=True)
class Val:
    address: bytes
    power: int
    priority: int = 0
    key: bytes = b""
    kind: int = 0

    def __str__(self):  # types/validator.go:129-138
        return "Validator{%s PubKey%s{%s} VP:%d A:%d}" % (self.address.hex().upper(), KIND_NAMES.get(self.kind, ""),
                                                         self.key.hex().upper(), self.power, self.priority)


def wrap(x: int) -> int:
    """An int64 result of Go's +, - or unary minus: two's complement."""
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def go_div(a: int, b: int) -> int:
    """Go's int64 /: truncation towards zero (Python's // floors), MinInt64 / -1 = MinInt64."""
    q = abs(a) // abs(b)
    return wrap(q if (a < 0) == (b < 0) else -q)


def safe_add_clip(a: int, b: int) -> int:
    return min(max(a + b, I64_MIN), I64_MAX)


def safe_sub_clip(a: int, b: int) -> int:
    return min(max(a - b, I64_MIN), I64_MAX)


def total_voting_power(vals) -> int:
    """updateTotalVotingPower."""
    s = 0
    for v in vals:
        s = safe_add_clip(s, v.power)
        if s > MAX_TOTAL_VOTING_POWER:
            raise ValsetPanic("Total voting power should be guarded to not exceed %d; got: %d" % (MAX_TOTAL_VOTING_POWER, s))
    return s


def max_min_priority_diff(vals) -> int:
    """computeMaxMinPriorityDiff: max - min as an int64 (it wraps), a negative result negated (-MinInt64 wraps back)."""
    diff = wrap(max(v.priority for v in vals) - min(v.priority for v in vals))
    return wrap(-diff) if diff < 0 else diff


def rescale_priorities(vals, diff_max: int):
    if not vals:
        raise ValsetPanic("empty validator set")
    if diff_max <= 0:
        return list(vals)
    diff = max_min_priority_diff(vals)
    ratio = go_div(wrap(diff + diff_max - 1), diff_max)
    if diff > diff_max:
        return [replace(v, priority=go_div(v.priority, ratio)) for v in vals]
    return list(vals)


def avg_proposer_priority(vals) -> int:
    """computeAvgProposerPriority: big.Int.Div is Euclidean division, the floor for the positive divisor."""
    return sum(v.priority for v in vals) // len(vals)


def shift_by_avg(vals):
    if not vals:
        raise ValsetPanic("empty validator set")
    avg = avg_proposer_priority(vals)
    return [replace(v, priority=safe_sub_clip(v.priority, avg)) for v in vals]


def most_priority(vals) -> int:
    """getValWithMostPriority: the index of the highest priority, ties to the smaller address."""
    best = 0
    for i, v in enumerate(vals):
        b = vals[best]
        if v.priority > b.priority or (v.priority == b.priority and v.address < b.address):
            best = i
    return best


def increment_proposer_priority(vals, times: int):
    """IncrementProposerPriority(times) -> (new set, proposer's index)."""
    if not vals:
        raise ValsetPanic("empty validator set")
    if times <= 0:
        raise ValsetPanic("Cannot call IncrementProposerPriority with non-positive times")
    total = total_voting_power(vals)
    vals = shift_by_avg(rescale_priorities(vals, PRIORITY_WINDOW_SIZE_FACTOR * total))
    prop = -1
    for _ in range(times):
        vals = [replace(v, priority=safe_add_clip(v.priority, v.power)) for v in vals]
        prop = most_priority(vals)
        vals[prop] = replace(vals[prop], priority=safe_sub_clip(vals[prop].priority, total))
    return vals, prop


def _list(vals) -> str:
    return "[" + " ".join(str(v) for v in vals) + "]"


def _get(vals, address):
    for v in vals:
        if v.address == address:
            return v
    return None


def update_with_change_set(vals, changes, allow_deletes: bool = True):
    """updateWithChangeSet -> the new set."""
    if not changes:
        return list(vals)
    changes = sorted(changes, key=lambda c: c.address)
    updates, deletes = [], []
    prev = b""
    for c in changes:
        if c.address == prev:
            raise ValsetError("duplicate entry %s in %s" % (c, _list(changes)))
        if c.power < 0:
            raise ValsetError("voting power can't be negative: %d" % c.power)
        if c.power > MAX_TOTAL_VOTING_POWER:
            raise ValsetError("to prevent clipping/overflow, voting power can't be higher than %d, got %d"
                              % (MAX_TOTAL_VOTING_POWER, c.power))
        (deletes if c.power == 0 else updates).append(c)
        prev = c.address
    if not allow_deletes and deletes:
        raise ValsetError("cannot process validators with voting power 0: %s" % _list(deletes))
    if not any(_get(vals, u.address) is None for u in updates) and len(vals) == len(deletes):
        raise ValsetError("applying the validator changes would result in empty set")
    removed = 0
    for d in deletes:
        v = _get(vals, d.address)
        if v is None:
            raise ValsetError("failed to find validator %s to remove" % d.address.hex().upper())
        removed += v.power
    if len(deletes) > len(vals):
        raise ValsetPanic("more deletes than validators")

    def delta(u):
        v = _get(vals, u.address)
        return u.power - v.power if v is not None else u.power
    tvp = total_voting_power(vals) - removed
    for d in sorted(delta(u) for u in updates):
        tvp += d
        if tvp > MAX_TOTAL_VOTING_POWER:
            raise ValsetError("total voting power of resulting valset exceeds max %d" % MAX_TOTAL_VOTING_POWER)
    tvp += removed
    fresh = []
    for u in updates:
        v = _get(vals, u.address)
        fresh.append(replace(u, priority=v.priority if v is not None else -(tvp + (tvp >> 3))))
    gone = {d.address for d in deletes}
    changed = {u.address for u in fresh}
    merged = [v for v in vals if v.address not in changed] + fresh
    merged = [v for v in merged if v.address not in gone]
    total = total_voting_power(merged)
    merged = shift_by_avg(rescale_priorities(merged, PRIORITY_WINDOW_SIZE_FACTOR * total))
    return sorted(merged, key=lambda v: (-v.power, v.address))


def new_validator_set(valz):
    """NewValidatorSet -> (set, proposer's index or -1)."""
    try:
        vals = update_with_change_set([], valz, False)
    except ValsetError as e:
        raise ValsetPanic("cannot create validator set: %s" % e)
    if not valz:
        return vals, -1
    return increment_proposer_priority(vals, 1)


def address_of(kind: int, key: bytes) -> bytes:
    """PubKey.Address()."""
    from vote_ext_ref import ripemd160  # hashlib's depends on the OpenSSL build
    d = hashlib.sha256(key).digest()
    return ripemd160(d) if kind == 3 else d[:20]
