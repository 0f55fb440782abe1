"""CPU: the conditions tests/golden/unitig_clean.json must meet (tools/make_unitig_clean_golden.py asserts them only when it is
run): every case cleans something, so that a route that cleans nothing cannot pass the GPU tests that compare against it."""
import json
import os

import golden_util as gu

with open(os.path.join(gu.GOLD, "unitig_clean.json")) as f:
    GOLDEN = json.load(f)["cases"]


def test_golden_cases_clean_something():
    assert len(GOLDEN) >= 10
    for c in GOLDEN:
        assert c["log"]["disconnected"][0] > 0, c["name"]
        assert len(c["log"]["disconnected"]) == c["log"]["rounds_run"] <= c["rounds"], c["name"]
        if c["rounds"] > 1 and c["opts"][:2] != ["--max_tip_len", "0"]:
            assert sum(c["log"]["tips"]) > 0, c["name"]
        assert len(c["digests"]) == 6, c["name"]


def test_golden_cases_cover_loops():
    by_name = {c["name"]: c["log"] for c in GOLDEN}
    assert by_name["A-plasmid"]["looped_before"] == 1 and by_name["A-plasmid"]["final"]["looped"] == 0  # a loop deleted as a tip
    assert by_name["C"]["looped_before"] == 0 and by_name["C"]["final"]["looped"] == 1  # a cycle merged by Refresh
    assert by_name["selfrc-circle"]["final"] == {"contigs": 1, "isolated": 1, "looped": 1}  # ... one that is its own reverse complement
