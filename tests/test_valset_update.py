"""The validator-set arithmetic (tendermint_amd/csrc/host/valset_update.h and its
C-ABI, tm_valset_abi.cpp) on the CPU: the host layer built without the engine
(tests/native/valset, libvalsethost.so) against the values of the reference's
own tests (tests/golden/validator_updates.json) and against the restatement in
unbounded integers (tests/valset_update_ref.py)."""
import ctypes
import json
import os
import random
import subprocess
from dataclasses import replace

import pytest

import valset_script as S
import valset_update_ref as R
from tendermint_amd import host as H
from valset_update_ref import I64_MAX, I64_MIN, MAX_TOTAL_VOTING_POWER as MAX_TVP, Val

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "_build", "libvalsethost.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "validator_updates.json")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = H._setup_valset(ctypes.CDLL(LIB))
    vp = ctypes.POINTER(H.CValidator)
    L.vs_update_by_address.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_int, vp,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
                                       ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def host_set(vals, prop=-1):
    return H.ValidatorSet([H.Validator(v.address, v.key, v.power, v.kind, v.priority) for v in vals], prop)


def ref_set(vs):
    return [Val(v.address, v.voting_power, v.proposer_priority, v.pub_key, v.key_kind) for v in vs.validators]


class CImpl:
    """valset_script's implementation over the C++ functions, the validators named by address."""

    def __init__(self, lib):
        self.lib = lib

    def _by_address(self, vals, changes, is_new):
        k = H._Keep()
        cv, cc = H._c_validators(k, host_set(vals)), H._c_validators(k, host_set(changes))
        out = (H.CValidator * max(1, len(vals) + len(changes)))()
        n, prop = ctypes.c_uint32(0), ctypes.c_int32(-1)
        err = ctypes.create_string_buffer(4096)
        rc = self.lib.vs_update_by_address(cv, len(vals), cc, len(changes), is_new, out, ctypes.byref(n),
                                           ctypes.byref(prop), err, len(err))
        if rc == H.VALSET_ERROR:
            raise R.ValsetError(err.value.decode())
        if rc == H.VALSET_PANIC:
            raise R.ValsetPanic(err.value.decode())
        assert rc == 0
        return [Val(ctypes.string_at(o.address, o.address_len), o.voting_power, o.proposer_priority)
                for o in out[:n.value]], prop.value

    def new(self, changes):
        return self._by_address([], changes, 1)

    def update(self, vals, changes):
        return self._by_address(vals, changes, 0)[0]

    def inc(self, vals, times):
        after, props = H.validator_set_rotate(host_set(vals), 1, times, lib=self.lib)
        return ref_set(after), props[0]


def test_golden_file_is_what_its_generator_writes(cases):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vu", os.path.join(REPO, "tests", "golden",
                                                                          "make_validator_updates_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.CASES == cases
    sources = {c["source"] for c in cases}
    assert sources == {"TestProposerSelection1", "TestProposerSelection2",
                       "TestAveragingInIncrementProposerPriorityWithVotingPower", "TestValSetUpdatesBasicTestsExecute",
                       "TestValSetUpdatePriorityOrderTests", "TestValSetUpdateOverflowRelated",
                       "TestValSetUpdatesDuplicateEntries", "TestValSetUpdatesOverflows", "TestValSetUpdatesOtherErrors"}


def test_golden_cpp(lib, cases):
    """The C++ functions reproduce every value the reference's tests assert."""
    impl = CImpl(lib)
    for c in cases:
        try:
            S.run_script(impl, c["script"])
        except AssertionError as e:
            raise AssertionError("%s / %s: %s" % (c["source"], c["name"], e))


def test_golden_restatement(cases):
    """So does the restatement, which the random comparisons below rely on."""
    for c in cases:
        S.run_script(S.RefImpl, c["script"])


# ---- the restatement against the C-ABI, validators named by key ----
def _key(rng, kind):
    return bytes(rng.randrange(256) for _ in range(33 if kind == 3 else 32))


def _member(rng, power=None, priority=None):
    kind = rng.choice([0, 0, 1, 3])
    key = _key(rng, kind)
    return Val(R.address_of(kind, key), rng.randint(1, 1000) if power is None else power,
               rng.randint(-5000, 5000) if priority is None else priority, key, kind)


def c_update(lib, vals, changes, allow_deletes=True):
    """(new set as Vals, None) or (None, (code, text)) through host.validator_set_update."""
    try:
        got, err = H.validator_set_update(host_set(vals), [(c.kind, c.key, c.power) for c in changes], allow_deletes, lib)
    except H.ValidatorSetPanic as e:
        return None, (2, str(e))
    return (ref_set(got), None) if err is None else (None, (1, err))


def ref_update(vals, changes, allow_deletes=True):
    try:
        return R.update_with_change_set(vals, changes, allow_deletes), None
    except R.ValsetError as e:
        return None, (1, str(e))
    except R.ValsetPanic as e:
        return None, (2, str(e))


def c_rotate(lib, vals, steps, times=1):
    try:
        after, props = H.validator_set_rotate(host_set(vals), steps, times, lib)
    except H.ValidatorSetPanic as e:
        return None, str(e)
    return ref_set(after), props


def ref_rotate(vals, steps, times=1):
    props = []
    try:
        for _ in range(steps):
            vals, p = R.increment_proposer_priority(vals, times)
            props.append(p)
    except R.ValsetPanic as e:
        return None, str(e)
    return vals, props


def same_update(lib, vals, changes, allow_deletes=True):
    want = ref_update(vals, changes, allow_deletes)
    assert c_update(lib, vals, changes, allow_deletes) == want
    return want


def same_rotate(lib, vals, steps, times=1):
    want = ref_rotate(vals, steps, times)
    assert c_rotate(lib, vals, steps, times) == want
    return want


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences(lib, seed):
    """Seeded sequences of change sets and rotations from sets of 1, 2 and more
    validators: powers changed, validators removed (the proposer among them) and
    added, now and then a change set the reference refuses."""
    rng = random.Random(seed)
    vals, _ = R.new_validator_set([_member(rng) for _ in range((1, 2, 3, 7, 20, 60)[seed])])
    for step in range(40):
        vals, props = same_rotate(lib, vals, rng.randint(1, 4), rng.choice([1, 1, 1, 2, 5]))
        prop = vals[props[-1]]
        changes = []
        for v in rng.sample(vals, rng.randint(0, min(3, len(vals)))):
            changes.append(Val(v.address, rng.choice([0, 0, rng.randint(1, 2000)]), 0, v.key, v.kind))
        if rng.random() < 0.3 and prop.address not in {c.address for c in changes}:
            changes.append(Val(prop.address, 0, 0, prop.key, prop.kind))  # the current proposer leaves
        changes += [_member(rng, priority=0) for _ in range(rng.randint(0, 3))]
        if rng.random() < 0.15 and changes:
            bad = rng.choice(["dup", "negative", "huge", "unknown"])
            if bad == "dup":
                changes.append(changes[0])
            elif bad == "negative":
                changes.append(_member(rng, power=-rng.randint(1, 9)))
            elif bad == "huge":
                changes.append(_member(rng, power=MAX_TVP + rng.randint(1, 9)))
            else:
                changes.append(_member(rng, power=0))
        rng.shuffle(changes)
        got, err = same_update(lib, vals, changes)
        if err is None:
            vals = got
            S.verify_validator_set(vals)


def _fixed(n, powers, prios, seed=5):
    rng = random.Random(seed)
    return [_member(rng, powers[i % len(powers)], prios[i % len(prios)]) for i in range(n)]


EDGE_SETS = {
    "one": _fixed(1, [7], [0]),
    "one_at_min": _fixed(1, [7], [I64_MIN]),
    "two_equal": _fixed(2, [5], [0]),
    "equal_priorities": _fixed(5, [3, 9], [11]),
    # clipping and the wrapped difference: max - min wraps to a negative int64
    "near_both_ends": _fixed(4, [10, 1], [I64_MAX - 2, I64_MIN + 3, I64_MAX, I64_MIN]),
    "difference_is_2_63": _fixed(2, [10], [I64_MAX, -1]),   # max - min = 2^63: -MinInt64 stays MinInt64, no rescale
    "difference_just_fits": _fixed(2, [10], [I64_MAX, 0]),  # diff + diffMax - 1 wraps: a negative ratio
    "near_max": _fixed(3, [1000], [I64_MAX - 1, I64_MAX - 5, I64_MAX]),
    "near_min": _fixed(3, [1000], [I64_MIN + 1, I64_MIN + 5, I64_MIN]),
    # floor and truncation differ: the sum is -7 over 3 validators (floor -3, truncation -2)
    "negative_sum": _fixed(3, [10], [-5, -3, 1]),
    "negative_sum_large": _fixed(3, [1 << 40], [-(1 << 62), -(1 << 62) - 1, -(1 << 62)]),
    # a rescale ratio above 1 over negative priorities: -7 / 2 is -3 in Go, -4 under a floor
    "negative_under_ratio": _fixed(4, [1], [-7, 9, -1, 3]),
    "negative_under_ratio_3": _fixed(3, [2], [-25, 10, -11]),
    # the elections of one call spread the priorities past 2 * total power: a second call rescales again
    "rescaled_again": [replace(v, power=p) for v, p in zip(_fixed(3, [1], [37, -31, 48]), (17, 1, 2))],
    "power_at_max": _fixed(2, [MAX_TVP - 1, 1], [0]),
    "power_above_max": _fixed(2, [MAX_TVP, 1], [0]),
}


@pytest.mark.parametrize("name", sorted(EDGE_SETS))
def test_rotate_edges(lib, name):
    vals = EDGE_SETS[name]
    for steps, times in ((1, 1), (3, 1), (1, 3), (2, 7)):
        same_rotate(lib, vals, steps, times)
    same_rotate(lib, vals, 1, 0)
    same_rotate(lib, vals, 1, -1)
    if name == "power_above_max":
        assert "Total voting power should be guarded" in ref_rotate(vals, 1)[1]


@pytest.mark.parametrize("name", sorted(EDGE_SETS))
def test_update_edges(lib, name):
    vals = EDGE_SETS[name]
    rng = random.Random(9)
    first, last = vals[0], vals[-1]
    for changes in ([Val(first.address, first.power + 1, 0, first.key, first.kind)],
                    [Val(last.address, 0, 0, last.key, last.kind), _member(rng, 3, 0)],
                    [_member(rng, 1, 0)],
                    [_member(rng, MAX_TVP, 0)],
                    # everyone leaves and one joins
                    [Val(v.address, 0, 0, v.key, v.kind) for v in vals] + [_member(rng, 4, 0)],
                    [Val(v.address, 0, 0, v.key, v.kind) for v in vals]):
        same_update(lib, vals, changes)
        same_update(lib, vals, changes, allow_deletes=False)


def test_the_traps_are_in_the_cases():
    """The inputs above do what their comments say, in the restatement's own terms."""
    ns = EDGE_SETS["negative_sum"]
    s = sum(v.priority for v in ns)
    assert s < 0 and s % len(ns) != 0 and R.avg_proposer_priority(ns) == -3 != int(s / len(ns))
    nr = EDGE_SETS["negative_under_ratio"]
    diff, diff_max = R.max_min_priority_diff(nr), 2 * R.total_voting_power(nr)
    assert diff > diff_max and (diff + diff_max - 1) // diff_max == 2
    assert [v.priority for v in R.rescale_priorities(nr, diff_max)] == [-3, 4, 0, 1]  # a floor gives -4 and -1
    assert R.go_div(-7, 2) == -3 and -7 // 2 == -4
    ne = EDGE_SETS["near_both_ends"]
    assert max(v.priority for v in ne) - min(v.priority for v in ne) > I64_MAX
    assert R.max_min_priority_diff(ne) == 1  # 2^64 - 1 wraps to -1, negated
    assert R.max_min_priority_diff(EDGE_SETS["difference_is_2_63"]) == I64_MIN
    dj = EDGE_SETS["difference_just_fits"]
    assert R.go_div(R.wrap(R.max_min_priority_diff(dj) + 40 - 1), 40) < 0
    assert R.safe_add_clip(I64_MAX - 2, 10) == I64_MAX and R.safe_sub_clip(I64_MIN + 3, 10) == I64_MIN
    assert R.total_voting_power(EDGE_SETS["power_at_max"]) == MAX_TVP
    with pytest.raises(R.ValsetPanic):
        R.total_voting_power(EDGE_SETS["power_above_max"])


def test_total_power_at_the_limit(lib):
    rng = random.Random(3)
    vals, _ = R.new_validator_set([_member(rng, MAX_TVP - 10, 0), _member(rng, 5, 0)])
    got, err = same_update(lib, vals, [_member(rng, 5, 0)])             # exactly MaxTotalVotingPower
    assert err is None and R.total_voting_power(got) == MAX_TVP
    same_rotate(lib, got, 3)
    got, err = same_update(lib, vals, [_member(rng, 6, 0)])             # one above
    assert err == (1, "total voting power of resulting valset exceeds max %d" % MAX_TVP)


def test_error_texts(lib):
    rng = random.Random(4)
    a, b, c = (_member(rng, 10, 0) for _ in range(3))
    vals, _ = R.new_validator_set([a, b])
    texts = {
        "dup": same_update(lib, vals, [Val(a.address, 3, 0, a.key, a.kind)] * 2)[1],
        "neg": same_update(lib, vals, [Val(a.address, -4, 0, a.key, a.kind)])[1],
        "high": same_update(lib, vals, [Val(c.address, MAX_TVP + 1, 0, c.key, c.kind)])[1],
        "empty": same_update(lib, vals, [Val(v.address, 0, 0, v.key, v.kind) for v in (a, b)])[1],
        "unknown": same_update(lib, vals, [Val(c.address, 0, 0, c.key, c.kind)])[1],
        "zero": same_update(lib, [], [Val(c.address, 0, 0, c.key, c.kind)], allow_deletes=False)[1],
    }
    assert texts["dup"][1].startswith("duplicate entry Validator{%s PubKey" % a.address.hex().upper())
    assert texts["dup"][1].count("Validator{") == 3 and texts["dup"][1].endswith("}]")
    assert texts["neg"] == (1, "voting power can't be negative: -4")
    assert texts["high"] == (1, "to prevent clipping/overflow, voting power can't be higher than %d, got %d"
                             % (MAX_TVP, MAX_TVP + 1))
    assert texts["empty"] == (1, "applying the validator changes would result in empty set")
    assert texts["unknown"] == (1, "failed to find validator %s to remove" % c.address.hex().upper())
    assert texts["zero"][1].startswith("cannot process validators with voting power 0: [Validator{")


def test_new_validator_set(lib):
    rng = random.Random(6)
    members = [_member(rng, priority=0) for _ in range(9)]
    want, prop = R.new_validator_set(members)
    got = H.new_validator_set([(m.kind, m.key, m.power) for m in members], lib)
    assert (ref_set(got), got.proposer_index) == (want, prop)
    assert [v.address for v in got.validators] == [R.address_of(v.key_kind, v.pub_key) for v in got.validators]
    empty = H.new_validator_set([], lib)
    assert empty.validators == [] and empty.proposer_index == -1
    with pytest.raises(H.ValidatorSetPanic, match="cannot create validator set: cannot process validators with"):
        H.new_validator_set([(0, members[0].key, 0)], lib)


def test_one_call_of_k_is_not_k_calls(lib):
    """IncrementProposerPriority(3) centres once; three calls centre three times."""
    vals = EDGE_SETS["rescaled_again"]
    assert same_rotate(lib, vals, 1, 3)[0] != same_rotate(lib, vals, 3, 1)[0]


def test_the_input_set_is_left_alone(lib):
    rng = random.Random(8)
    vals, _ = R.new_validator_set([_member(rng) for _ in range(4)])
    hs = host_set(vals)
    before = [(v.address, v.voting_power, v.proposer_priority) for v in hs.validators]
    H.validator_set_rotate(hs, 5, lib=lib)
    H.validator_set_update(hs, [(0, _key(rng, 0), 5)], lib=lib)
    assert [(v.address, v.voting_power, v.proposer_priority) for v in hs.validators] == before


def test_set_hash_on_the_host(lib):
    from tendermint_amd.testing.factory import _valset_hash
    rng = random.Random(2)
    vals = [_member(rng) for _ in range(7)]
    assert any(v.kind == 3 for v in vals)
    assert H.validator_set_hash_host(host_set(vals), lib) == _valset_hash(host_set(vals))


def test_valset_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "valset"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "valset_san"), GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
