"""Runs the scripts of tests/golden/validator_updates.json (the language is
described in tests/golden/make_validator_updates_golden.py) over an
implementation of the validator-set arithmetic: an object with
  new(changes) -> (vals, proposer's index)
  inc(vals, times) -> (vals, proposer's index)
  update(vals, changes) -> vals          (raises valset_update_ref.ValsetError)
over lists of valset_update_ref.Val.  RefImpl is the restatement itself."""
import valset_update_ref as R
from valset_update_ref import Val


class RefImpl:
    new = staticmethod(R.new_validator_set)
    inc = staticmethod(R.increment_proposer_priority)
    update = staticmethod(R.update_with_change_set)


def _addr(tok: str) -> bytes:
    return bytes.fromhex(tok[2:]) if tok.startswith("0x") else tok.encode()


def _val(tok: str) -> Val:
    f = tok.split(":")
    return Val(_addr(f[0]), int(f[1]), int(f[2]) if len(f) > 2 else 0)


def _pairs(vals):
    return [(v.address, v.power) for v in vals]


def verify_validator_set(vals):
    """verifyValidatorSet (types/validator_set_test.go:774-795)."""
    tvp = R.total_voting_power(vals)
    tpp = 0
    for v in vals:
        tpp = R.safe_add_clip(tpp, v.priority)
    assert -len(vals) < tpp < len(vals), "priorities not centred: %d" % tpp
    assert R.max_min_priority_diff(vals) <= R.PRIORITY_WINDOW_SIZE_FACTOR * tvp, "priorities not scaled"


def run_script(impl, script: str):
    """Asserts every expectation of the script; returns the final set."""
    vals, prop = [], -1
    for step in script.split("; "):
        op, *args = step.split(" ")
        if op == "new":
            vals, prop = impl.new([_val(a) for a in args])
        elif op == "raw":
            vals, prop = [_val(a) for a in args], -1
        elif op == "inc":
            vals, prop = impl.inc(vals, int(args[0]))
        elif op == "upd":
            vals = impl.update(vals, [_val(a) for a in args])
        elif op == "upd!":
            try:
                impl.update(vals, [_val(a) for a in args])
            except R.ValsetError:
                pass
            else:
                raise AssertionError("no error: " + step)
        elif op == "vals":
            assert _pairs(vals) == _pairs(_val(a) for a in args), step
        elif op == "prios":
            assert [v.priority for v in vals] == [int(a) for a in args], step
        elif op == "prop":
            assert vals[prop].address == _addr(args[0]), step
        elif op == "seq":
            got = []
            for _ in range(int(args[0])):
                got.append(vals[prop].address)
                vals, prop = impl.inc(vals, 1)
            assert got == [_addr(a) for a in args[1:]], step
        elif op == "count":
            got = {}
            for _ in range(int(args[0])):
                got[vals[prop].address] = got.get(vals[prop].address, 0) + 1
                vals, prop = impl.inc(vals, 1)
            assert got == {_addr(a.split(":")[0]): int(a.split(":")[1]) for a in args[1:]}, step
        elif op == "verify":
            verify_validator_set(vals)
        elif op == "added":
            added = {_addr(a) for a in args}
            lowest = min(v.priority for v in vals)
            assert added <= {v.address for v in vals if v.priority == lowest}, step
        else:
            raise ValueError("unknown step " + step)
    return vals
