"""CPU: tests/golden/unitig_prune.json (tools/make_unitig_prune_golden.py) is well-formed and covers the case list — every
option set of the low-depth pruning route, each one removing something in the step it is there for."""
import json
import os
import re
import sys

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_prune_golden as mpg  # noqa: E402

with open(os.path.join(gu.GOLD, "unitig_prune.json")) as f:
    CASES = json.load(f)["cases"]


def test_the_committed_cases_are_the_generators():
    keys = [k for k in mpg.CASES[0]]
    assert [{k: c.get(k) for k in keys} for c in CASES] == [{k: c.get(k) for k in keys} for c in mpg.CASES]
    assert [c.get("plasmid") for c in CASES] == [c.get("plasmid") for c in mpg.CASES]
    assert len({c["name"] for c in CASES}) == len(CASES)


def test_every_case_has_eight_digests_and_its_counts():
    assert len(mpg.FILES) == 8 and ".addi.fa" in mpg.FILES and ".addi.fa.info" in mpg.FILES
    for c in CASES:
        assert sorted(c["digests"]) == sorted(mpg.FILES), c["name"]
        assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in c["digests"].values()), c["name"]
        log = c["log"]
        assert log["low_depth_removed"] > 0, c["name"]  # a case that prunes nothing shows nothing
        assert len(log["pruned"]) == (log["rounds_run"] if c["prune"] == 2 else 0), c["name"]
        assert log["rounds_run"] == len(log["disconnected"]) and (c["rounds"] > 0) == (log["rounds_run"] > 0), c["name"]
        assert log["addi_records"] == 0 or not c["final"], c["name"]
        assert 6000 <= c["G"] <= 20000 or c["kind"] == "selfrc-circular"
        assert c["pairs"] <= 6000 and 21 <= c["k"] <= 63


def test_the_case_list_is_covered():
    def has(pred):
        return any(pred(c) for c in CASES)

    for prune in (1, 2):
        for final in (False, True):
            assert has(lambda c: c["prune"] == prune and c["final"] == final and c["rounds"] > 0 and not c["opts"])
    assert has(lambda c: c["rounds"] == 0 and c["prune"] == 1)
    assert has(lambda c: c["opts"][:3] == ["--output_standalone", "--min_standalone", "0"])
    assert has(lambda c: c["opts"][:2] == ["--low_local_ratio", "0.05"] and c["prune"] == 2 and sum(c["log"]["pruned"]) > 0)
    assert has(lambda c: c["m"] == 1 and c["min_depth"] == 2 and sum(c["log"]["pruned"]) > 0)
    for kind in ("circular", "palindrome", "linear+plasmid", "selfrc-circular"):
        assert has(lambda c: c["kind"] == kind)
    assert has(lambda c: c["k"] == 21) and has(lambda c: c["k"] == 63)
    assert has(lambda c: not c["final"] and c["log"]["addi_records"] > 0)
    assert has(lambda c: c["final"] and c["contigs_differ_from_prune0"])
    assert has(lambda c: c["log"]["final"]["looped"] == 1 and c["log"]["addi_records"] == 1)  # a merged cycle is a changed contig
