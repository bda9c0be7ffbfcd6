"""Writes tests/golden/validator_updates.json from the literal data below: the
inputs and expected outputs of the reference's own validator-set tests
(types/validator_set_test.go), transcribed as data.  They are the only values
made by the reference's code that this repository holds for the validator-set
arithmetic (tendermint_amd/csrc/host/valset_update.h).

Each case is a script, steps separated by "; ", read by tests/valset_script.py
and by tests/native/valset/valset_san.cpp.  A validator is address:power (or
address:power:priority for `raw`); an address is its ASCII name, or 0x and hex.
  new V...        NewValidatorSet(V...)
  raw V...        ValidatorSet{Validators: V...}, as a literal (no proposer)
  inc T           IncrementProposerPriority(T)
  upd V...        UpdateWithChangeSet(V...) returns no error
  upd! V...       UpdateWithChangeSet(V...) returns an error, the set is unchanged
  vals V...       the set holds exactly V..., in this order
  prios P...      the priorities, in set order
  prop A          GetProposer().Address
  seq N A...      N times: GetProposer().Address is the next A, then IncrementProposerPriority(1)
  count N A:C...  over N such rounds A proposes C times
  verify          verifyValidatorSet: the total power is the sum, the priorities sum to within
                  (-n, n), and max - min <= 2 * total power
  added A...      the validators A... hold the smallest priority of the set, all the same one

Usage: python3 tests/golden/make_validator_updates_golden.py"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_TVP = ((1 << 63) - 1) // 8  # MaxTotalVotingPower
I64_MAX = (1 << 63) - 1


def vl(pairs):
    return " ".join("%s:%d" % p for p in pairs)


def tvs(n, power):  # testValSet
    return [("v%d" % (i + 1), power) for i in range(n)]


CASES = []


def case(source, name, *steps):
    CASES.append({"source": source, "name": name, "script": "; ".join(steps)})


# ---- TestProposerSelection1
SELECTION1 = ("foo baz foo bar foo foo baz foo bar foo foo baz foo foo bar foo baz foo foo bar"
              " foo foo baz foo bar foo foo baz foo bar foo foo baz foo foo bar foo baz foo foo bar"
              " foo baz foo foo bar foo baz foo foo bar foo baz foo foo foo baz bar foo foo foo baz"
              " foo bar foo foo baz foo bar foo foo baz foo bar foo foo baz foo bar foo foo baz foo"
              " foo bar foo baz foo foo bar foo baz foo foo bar foo baz foo foo")
case("TestProposerSelection1", "99 proposers", "new foo:1000 bar:300 baz:330", "seq 99 " + SELECTION1)

# ---- TestProposerSelection2
A0, A1, A2 = ("0x" + "00" * 19 + "%02x" % i for i in range(3))
case("TestProposerSelection2", "equal power goes in order of addresses", "new %s:100 %s:100 %s:100" % (A0, A1, A2),
     "seq 15 " + " ".join([A0, A1, A2] * 5))
case("TestProposerSelection2", "more power, not twice in a row", "new %s:100 %s:100 %s:400" % (A0, A1, A2),
     "prop " + A2, "inc 1", "prop " + A0)
case("TestProposerSelection2", "enough power to propose twice in a row", "new %s:100 %s:100 %s:401" % (A0, A1, A2),
     "prop " + A2, "inc 1", "prop " + A2, "inc 1", "prop " + A0)
case("TestProposerSelection2", "proportional counts", "new %s:4 %s:5 %s:3" % (A0, A1, A2),
     "count 120 %s:40 %s:50 %s:30" % (A0, A1, A2))

# ---- TestAveragingInIncrementProposerPriorityWithVotingPower: times -> (priorities, proposer's index)
AVERAGING = {1: ([-2, 1, 1], 0), 2: ([-4, 2, 2], 0), 3: ([-6, 3, 3], 0), 4: ([-8, 4, 4], 0), 5: ([2, -7, 5], 1),
             6: ([0, -6, 6], 0), 7: ([-2, -5, 7], 0), 8: ([-4, -4, 8], 0), 9: ([6, -3, -3], 2), 10: ([4, -2, -2], 0),
             11: ([2, -1, -1], 0)}
for times, (prios, prop) in AVERAGING.items():
    case("TestAveragingInIncrementProposerPriorityWithVotingPower", "times %d" % times, "raw 0x00:10:0 0x01:1:0 0x02:1:0",
         "inc %d" % times, "prop 0x%02x" % prop, "prios " + " ".join(map(str, prios)))

# ---- TestValSetUpdatesBasicTestsExecute: (start, update, expected)
BASIC = [
    ("no changes", tvs(2, 10), [], tvs(2, 10)),
    ("voting power changes", tvs(2, 10), [("v2", 22), ("v1", 11)], [("v2", 22), ("v1", 11)]),
    ("add new validators", [("v2", 20), ("v1", 10)], [("v4", 40), ("v3", 30)],
     [("v4", 40), ("v3", 30), ("v2", 20), ("v1", 10)]),
    ("add new validator to middle", [("v3", 20), ("v1", 10)], [("v2", 30)], [("v2", 30), ("v3", 20), ("v1", 10)]),
    ("add new validator to beginning", [("v3", 20), ("v2", 10)], [("v1", 30)], [("v1", 30), ("v3", 20), ("v2", 10)]),
    ("delete validators", [("v3", 30), ("v2", 20), ("v1", 10)], [("v2", 0)], [("v3", 30), ("v1", 10)]),
]
for name, start, update, expected in BASIC:
    case("TestValSetUpdatesBasicTestsExecute", name, "new " + vl(start), ("upd " + vl(update)).strip(),
         "vals " + vl(expected), "verify")

# ---- TestValSetUpdatePriorityOrderTests: the three literal configurations (the others are drawn at random
# by the reference's test); it draws the number of elections from 1..5000, here the ends and a few between
PRIORITY_ORDER = [
    ("remove high power validator, keep old equal lower power validators",
     [("v3", 1000), ("v1", 1), ("v2", 1)], [("v3", 0)], [], [], [("v1", 1), ("v2", 1)]),
    ("remove high power validator, keep old different power validators",
     [("v3", 1000), ("v2", 10), ("v1", 1)], [("v3", 0)], [], [], [("v2", 10), ("v1", 1)]),
    ("remove high power validator, add new low power validators, keep old lower power",
     [("v3", 1000), ("v2", 2), ("v1", 1)], [("v3", 0)], [("v2", 1)], [("v5", 50), ("v4", 40)],
     [("v5", 50), ("v4", 40), ("v1", 1), ("v2", 1)]),
]
for name, start, deleted, updated, added, expected in PRIORITY_ORDER:
    for times in (1, 2, 3, 17, 1000, 4999, 5000):
        steps = ["new " + vl(start), "verify", "inc %d" % times, "upd " + vl(added + updated + deleted),
                 "vals " + vl(expected), "verify"]
        if added:
            steps.append("added " + " ".join(a for a, _ in added))
        case("TestValSetUpdatePriorityOrderTests", "%s, %d elections" % (name, times), *steps)

# ---- TestValSetUpdateOverflowRelated: (name, start, deleted, updated, added, expected, error expected)
OVERFLOW_RELATED = [
    ("1 no false overflow error messages for updates", [("v2", MAX_TVP - 1), ("v1", 1)], [],
     [("v1", MAX_TVP - 1), ("v2", 1)], [], [("v1", MAX_TVP - 1), ("v2", 1)], False),
    ("2 no false overflow error messages for updates", [("v2", MAX_TVP - 1), ("v1", 1)], [],
     [("v1", MAX_TVP // 2 - 1), ("v2", MAX_TVP // 2)], [], [("v2", MAX_TVP // 2), ("v1", MAX_TVP // 2 - 1)], False),
    ("3 no false overflow error messages for deletes", [("v1", MAX_TVP - 2), ("v2", 1), ("v3", 1)], [("v1", 0)], [],
     [("v4", MAX_TVP - 2)], [("v4", MAX_TVP - 2), ("v2", 1), ("v3", 1)], False),
    ("4 no false overflow error messages for adds, updates and deletes",
     [("v1", MAX_TVP // 4), ("v2", MAX_TVP // 4), ("v3", MAX_TVP // 4), ("v4", MAX_TVP // 4)], [("v2", 0)],
     [("v1", MAX_TVP // 2 - 2), ("v3", MAX_TVP // 2 - 3), ("v4", 2)], [("v5", 3)],
     [("v1", MAX_TVP // 2 - 2), ("v3", MAX_TVP // 2 - 3), ("v5", 3), ("v4", 2)], False),
    ("5 check panic on overflow is prevented: update 8 validators with power int64(math.MaxInt64)/8",
     [("v%d" % i, 1) for i in range(1, 10)], [], [("v%d" % i, MAX_TVP) for i in range(1, 9)] + [("v9", 8)], [],
     [("v%d" % i, 1) for i in range(1, 10)], True),
]
for name, start, deleted, updated, added, expected, fails in OVERFLOW_RELATED:
    case("TestValSetUpdateOverflowRelated", name, "new " + vl(start), "verify",
         ("upd! " if fails else "upd ") + vl(added + updated + deleted), "vals " + vl(expected), "verify")

# ---- the error tables: (start, changes), every one an error that leaves the set unchanged
DUPLICATES = [
    (tvs(2, 10), [("v1", 11), ("v1", 22)]),
    (tvs(2, 10), [("v2", 11), ("v2", 22)]),
    (tvs(2, 10), [("v1", 11), ("v2", 22), ("v1", 12)]),
    (tvs(3, 10), [("v1", 11), ("v3", 22), ("v1", 12)]),
    (tvs(2, 10), [("v1", 0), ("v1", 0)]),
    (tvs(2, 10), [("v2", 0), ("v2", 0)]),
    (tvs(2, 10), [("v1", 0), ("v2", 0), ("v1", 0)]),
    (tvs(3, 10), [("v1", 0), ("v3", 0), ("v1", 0)]),
    (tvs(2, 10), [("v1", 0), ("v2", 20), ("v1", 30)]),
    (tvs(2, 10), [("v1", 0), ("v2", 20), ("v2", 30), ("v1", 0)]),
    (tvs(3, 10), [("v1", 0), ("v3", 5), ("v2", 20), ("v2", 30), ("v1", 0)]),
]
OVERFLOWS = [
    (tvs(2, 10), [("v1", I64_MAX)]),
    (tvs(2, 10), [("v2", I64_MAX)]),
    (tvs(1, MAX_TVP), [("v2", I64_MAX)]),
    (tvs(1, MAX_TVP - 1), [("v2", 5)]),
    (tvs(2, MAX_TVP // 3), [("v3", MAX_TVP // 2)]),
    (tvs(1, MAX_TVP), [("v2", MAX_TVP)]),
]
OTHER_ERRORS = [
    (tvs(2, 10), [("v1", -123)]),
    (tvs(2, 10), [("v2", -123)]),
    (tvs(2, 10), [("v3", 0)]),
    ([("v1", 10), ("v2", 20), ("v3", 30)], [("v1", 0), ("v2", 0), ("v3", 0)]),
]
for source, table in (("TestValSetUpdatesDuplicateEntries", DUPLICATES), ("TestValSetUpdatesOverflows", OVERFLOWS),
                      ("TestValSetUpdatesOtherErrors", OTHER_ERRORS)):
    for k, (start, changes) in enumerate(table):
        case(source, "case %d" % k, "new " + vl(start), "upd! " + vl(changes))


if __name__ == "__main__":
    path = os.path.join(HERE, "validator_updates.json")
    doc = {"comment": "written by make_validator_updates_golden.py; the script language is described there",
           "cases": CASES}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(path, len(CASES), "cases", os.path.getsize(path), "bytes")
