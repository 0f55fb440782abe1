"""CPU: tests/golden/assemble_fuzz.json (tools/fuzz_assemble.py --write-golden) is what the reference's `read2sdbg` + `assemble -t 1`
give today for every committed seed (needs oracle/_ref/ref_megahit_core), and the list as a whole, judged on the reference's
output alone, reaches the branches it is there for: loops before and after cleaning, palindromes, every kind of removal
(naive and complex bubbles in a round, the final complex pop, --careful_bubble records, .addi.fa records, unitig tips,
disconnections, low-depth removals at prune level 1 or 2, the pruning of level 3), empty graphs and graphs that leave no
contig, every k and every --max_tip_len of the generator, and multiplicities past the 8-bit field."""
import json
import os
import re
import shutil
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import fuzz_assemble as fa  # noqa: E402

with open(fa.GOLDEN) as f:
    CASES = json.load(f)["cases"]


def option(c, name):
    return c["args"][c["args"].index(name) + 1]


def reach(cases):
    """condition -> number of cases that meet it"""
    def count(pred):
        return sum(1 for c in cases if pred(c, c["log"]))

    def prune(c):
        return int(option(c, "--prune_level"))

    out = {
        "a: loop before cleaning": count(lambda c, g: g["looped_before"] > 0),
        "a: loop after cleaning": count(lambda c, g: g["final"]["looped"] > 0),
        "b: palindromes": count(lambda c, g: g["palindromes"] > 0),
        "c: naive bubbles": count(lambda c, g: sum(g["naive"]) > 0),
        "c: complex bubbles in a round": count(lambda c, g: sum(g["complex"]) > 0),
        "c: final complex pop": count(lambda c, g: g["final_pass"] is not None and g["final_pass"][1] > 0),
        "c: careful records": count(lambda c, g: g["bubble_seq_records"] > 0),
        "c: addi records": count(lambda c, g: g["addi_records"] > 0),
        "c: unitig tips": count(lambda c, g: sum(g["tips"]) > 0),
        "c: disconnections": count(lambda c, g: sum(g["disconnected"]) > 0),
        "c: low-depth removals at prune 1 or 2": count(lambda c, g: prune(c) in (1, 2) and g["final_pass"][0] + sum(g["pruned"]) > 0),
        "c: pruning of level 3": count(lambda c, g: prune(c) == 3 and sum(g["more_pruned"]) > 0),
        "d: empty unitig graph": count(lambda c, g: g["graph_size"] == 0),
        "d: non-empty graph, no contig": count(lambda c, g: g["graph_size"] > 0 and g["contigs_records"] + g["final_contigs_records"] + g["addi_records"] == 0),
        "f: multiplicity above 255": count(lambda c, g: c["max_mul"] > 255),
    }
    for k in fa.K_LIST:
        out["e: k = %d" % k] = count(lambda c, g: c["k"] == k)
    for i, name in enumerate(("-1", "0", "1", "2", "10", "k", "2k+1", "500")):
        out["e: --max_tip_len " + name] = count(lambda c, g: int(option(c, "--max_tip_len")) == fa.tip_lens(c["k"])[i])
    return out


NEEDED = {"a: loop before cleaning": 6, "a: loop after cleaning": 2, "b: palindromes": 6, "d: empty unitig graph": 2, "d: non-empty graph, no contig": 2,
          "f: multiplicity above 255": 3}


def needed(name):
    return NEEDED.get(name, 4 if name.startswith("c:") else 1)


def test_the_list_reaches_its_branches():
    got = reach(CASES)
    print(got)
    short = {name: (n, needed(name)) for name, n in got.items() if n < needed(name)}
    assert not short, short


def test_the_committed_cases_are_the_generators():
    assert len(CASES) == 32 and len({c["name"] for c in CASES}) == 32
    assert [(c["name"], c["seed"]) for c in CASES] == [tuple(x) for x in fa.COMMITTED]
    for c in CASES:
        made = fa.case(c["seed"])
        assert (made["k"], made["args"]) == (c["k"], c["args"]), c["name"]
        with_addi = int(option(c, "--prune_level")) >= 1  # .addi.fa: prune level >= 1
        assert sorted(c["digests"]) == sorted(s for s in fa.FILES if with_addi or not s.startswith(".addi")), c["name"]
        assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in c["digests"].values()), c["name"]
    assert os.path.getsize(fa.GOLDEN) < 60000


def test_only_option_sets_inside_the_similarity_cap_are_drawn():
    # at k = 255: 40 / 0.8 -> (12750 + 255) * 0.2 = 2601 indels >= 2048; 60 / 0.8 -> 19380 and 60 / 0.9 -> 17255 characters > 16384;
    # 60 / 0.95 -> 16360 characters, 818 indels: inside
    outside = {(40, "0.8"), (60, "0.8"), (60, "0.9")}
    assert set(fa.MERGE_PAIRS) == {(ml, s) for ml in fa.MERGE_LEN for s in fa.MERGE_SIMILAR} - outside
    for seed in range(200):
        c = fa.case(seed)
        assert (int(option(c, "--merge_len")), option(c, "--merge_similar")) in fa.MERGE_PAIRS
        assert c["read_len"] > c["k"] and sum(r["seq"].size for r in c["replicons"]) > 0


def test_a_case_is_its_seed_alone():
    a, b = fa.case(7), fa.case(7)
    assert a["args"] == b["args"] and (fa.reads_of(a) == fa.reads_of(b)).all()
    assert fa.reads_of(a).shape[0] * a["read_len"] <= 1500000


@pytest.mark.skipif(not os.path.exists(fa.REF), reason="oracle/_ref/ref_megahit_core not built (no reference sources here)")
def test_the_reference_still_gives_the_committed_answers():
    def again(c):
        d = tempfile.mkdtemp(prefix="fuzz_assemble_")
        try:
            return fa.reference_case(fa.case(c["seed"]), d)
        finally:
            shutil.rmtree(d, ignore_errors=True)

    with ThreadPoolExecutor(4) as pool:  # (the work is in child processes)
        for c, (dig, log, mul) in zip(CASES, pool.map(again, CASES)):
            assert (dig, log, mul) == (c["digests"], c["log"], c["max_mul"]), c["name"]


def test_the_comparison_sees_a_changed_file_a_missing_file_and_a_changed_count():
    c = CASES[1]
    ref = (c["digests"], c["log"])
    assert fa.differences(ref, (dict(c["digests"]), json.loads(json.dumps(c["log"])))) == []
    assert fa.differences((dict(c["digests"], **{".contigs.fa": "0" * 64}), c["log"]), ref) == [".contigs.fa"]
    assert fa.differences(({s: v for s, v in c["digests"].items() if s != ".bubble_seq.fa.info"}, c["log"]), ref) == [".bubble_seq.fa.info"]
    assert fa.differences((c["digests"], dict(c["log"], tips=c["log"]["tips"] + [1])), ref) == ["tips"]
    assert fa.differences((c["digests"], dict(c["log"], final=dict(c["log"]["final"], looped=99))), ref) == ["final"]
