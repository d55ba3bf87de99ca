"""Records, for every case of tests/record_entry_cases.py, the return code of the built library and -- for a pair case -- which of
its two single violations produced the same message (the check that wins; where both single messages equal the pair's, the
library states the two checks in one message and the earlier one is recorded) into tests/golden/record_entries.json.

Recorded at the commit BEFORE the entries' validation was rewritten on shared checks; tests/test_record_entries_host.py holds the
rewritten entries to it.  Run it again only for a new case, and review the diff.

    python tests/golden/gen_record_entries.py          (needs the built library, no GPU: no case reaches a launch)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from scalable_collision_avoidance_rl_amd import _native  # noqa: E402
from tests import record_entry_cases as RC  # noqa: E402


def main():
    lib = _native.lib()
    out, messages = {}, {}
    for case in RC.cases():
        rc, msg = RC.run(lib, case)
        assert rc in (_native.OK, _native.EINVAL), (case.entry, case.label, rc, msg)      # ELAUNCH: a case got as far as a launch
        messages[case.entry, case.label] = msg
        rec = out.setdefault(case.entry, {})[case.label] = {"code": rc}
        if case.pair:
            same = [label for label in case.pair if messages[case.entry, label] == msg]
            assert rc != 0 and same, (case.entry, case.label, msg)
            rec["winner"] = same[0]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "record_entries.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(sum(len(v) for v in out.values()), "cases,", sum("winner" in c for v in out.values() for c in v.values()), "pairs")


if __name__ == "__main__":
    main()
