"""Argument validation of the entries that read observation records -- the shield, the obstacle kernels and the safety tables -- on
the host (no GPU needed; no case reaches a launch): every case of tests/record_entry_cases.py returns the code recorded in
tests/golden/record_entries.json (by tests/golden/gen_record_entries.py, before the entries were rewritten on shared checks), every
message starts with the entry's own name, and where two adjacent checks are violated at once the recorded one still wins."""
import json
import os

import pytest

from scalable_collision_avoidance_rl_amd import _native
from tests import record_entry_cases as RC

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_entries.json")))
CASES = RC.cases()


def test_golden_and_cases_name_the_same_cases():
    assert {(c.entry, c.label) for c in CASES} == {(e, l) for e, v in GOLDEN.items() for l in v} and len(CASES) == 322
    assert set(GOLDEN) == {"dronesim_action_shield", "dronesim_action_shield_obstacles", "dronesim_shield_totals", "dronesim_obstacle_sense",
                           "dronesim_obstacle_observe", "dronesim_obstacle_reward", "dronesim_episode_obstacle_safety",
                           "dronesim_episode_safety"}
    for c in CASES:
        assert list(c.args) == list(RC.ENTRIES[c.entry].base) and len(c.args) + 1 == len(_native.SIGNATURES[c.entry].argtypes)
        # a case with a non-empty batch is one validation refuses (an accepted one would launch on fake pointers)
        batch = [c.args[n] for n in ("E", "R", "T") if n in c.args]
        assert min(batch) <= 0 or GOLDEN[c.entry][c.label]["code"] == _native.EINVAL, (c.entry, c.label)


@pytest.mark.parametrize("entry", list(RC.ENTRIES))
def test_codes_names_and_winners(entry):
    lib, want, messages = _native.lib(), GOLDEN[entry], {}
    for c in (c for c in CASES if c.entry == entry):
        rc, msg = RC.run(lib, c)
        assert rc == want[c.label]["code"], (c.label, rc, msg)
        assert rc == 0 or msg.startswith(entry + ": "), (c.label, msg)
        messages[c.label] = msg
        if c.pair:
            assert msg == messages[want[c.label]["winner"]], (c.label, msg)
            assert len({messages[l] for l in c.pair}) == 2 or want[c.label]["winner"] == c.pair[0]
    assert sum(1 for c in CASES if c.entry == entry and c.pair) >= len(RC.ENTRIES[entry].checks) - 1
