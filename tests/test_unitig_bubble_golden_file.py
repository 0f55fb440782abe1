"""CPU: tests/golden/unitig_bubble.json (tools/make_unitig_bubble_golden.py) is well-formed and covers the case list — bubble
levels 1 and 2, prune levels 0, 2 and 3, final and non-final rounds, with and without --careful_bubble, --merge_len 0, the
early return of the complex pass, and the graphs that are their own reverse complement — each one popping something in the
step it is there for."""
import json
import os
import re
import sys

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_bubble_golden as mbg  # noqa: E402

with open(os.path.join(gu.GOLD, "unitig_bubble.json")) as f:
    CASES = json.load(f)["cases"]
NOTHING_COMPLEX = ("A-b2-merge0", "A-b2-early-return", "A-b2-p0-sim0.98")


def test_the_committed_cases_are_the_generators():
    keys = sorted({k for c in mbg.CASES for k in c})
    assert [{k: c.get(k) for k in keys} for c in CASES] == [{k: c.get(k) for k in keys} for c in mbg.CASES]
    assert len({c["name"] for c in CASES}) == len(CASES)
    assert os.path.getsize(os.path.join(gu.GOLD, "unitig_bubble.json")) < 40000  # the size class of unitig_prune.json


def test_every_case_has_its_digests_and_counts():
    for c in CASES:
        files = mbg.FILES if c["prune"] >= 1 else [s for s in mbg.FILES if not s.startswith(".addi")]  # .addi.fa: prune level >= 1
        assert sorted(c["digests"]) == sorted(files), c["name"]
        assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in c["digests"].values()), c["name"]
        log = c["log"]
        assert log["rounds_run"] == len(log["disconnected"]) == len(log["naive"]) > 0, c["name"]
        assert sum(log["naive"]) > 0, c["name"]  # a case that pops nothing shows nothing
        assert len(log["complex"]) == (log["rounds_run"] if c["bubble"] >= 2 else 0), c["name"]
        if c["bubble"] >= 2:
            assert (sum(log["complex"]) == 0) == (c["name"] in NOTHING_COMPLEX), c["name"]
        assert len(log["more_pruned"]) == (log["rounds_run"] if c["prune"] == 3 else 0), c["name"]
        assert len(log["pruned"]) == (log["rounds_run"] if c["prune"] == 2 else 0), c["name"]
        assert (log["final_pass"] is None) == (c["prune"] == 0), c["name"]
        assert c["careful"] or log["bubble_records"] == 0, c["name"]
        assert log["addi_records"] == 0 or not c["final"], c["name"]


def test_the_case_list_is_covered():
    def has(pred):
        return any(pred(c) for c in CASES)

    for bubble in (1, 2):
        assert has(lambda c: c["bubble"] == bubble and c["careful"] and c["log"]["bubble_records"] > 0)
        assert has(lambda c: c["bubble"] == bubble and not c["careful"])
        assert has(lambda c: c["bubble"] == bubble and c["prune"] == 3 and sum(c["log"]["more_pruned"]) > 0)
        assert has(lambda c: c["bubble"] == bubble and c["final"])
    for prune in (0, 2, 3):
        assert has(lambda c: c["prune"] == prune)
    assert has(lambda c: c["final"] and sum(c["log"]["complex"]) > 0) and has(lambda c: not c["final"] and sum(c["log"]["complex"]) > 0)
    assert has(lambda c: c["log"]["final_pass"] and c["log"]["final_pass"][1] > 0)  # the final complex pop finds something
    assert has(lambda c: c["opts"][:2] == ["--merge_len", "0"] and c["log"]["final_pass"][1] == 0)
    assert has(lambda c: c["name"] == "A-b2-early-return" and sum(c["log"]["complex"]) == 0)
    # the same graph at 0.95 and at 0.98: what pops at 0.95 fails a similarity check at 0.98
    assert has(lambda c: c["name"] == "A-b2-p0-sim0.98") and has(lambda c: c["name"] == "A-b2" and sum(c["log"]["complex"]) > 0)
    for kind in ("diploid", "diploid-palindrome", "diploid-selfrc-circular"):
        assert has(lambda c: c["kind"] == kind and c["bubble"] == 2)
    assert has(lambda c: c["k"] == 21) and has(lambda c: c["k"] == 63) and has(lambda c: c["m"] == 1)
    assert has(lambda c: c["rounds"] == 1)
