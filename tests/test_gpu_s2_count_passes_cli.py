"""GPU: `mhx_core read2sdbg` plans stage 2 from a count of the (k+1)-mers in passes over the count's own lv1 bucket ranges (plan_s2_count_passes
in host/mhx_core.cpp; MHX_S2_COUNT_PASSES=0 switches it off) where one run of that route does not fit the (faked) free device memory: the log line
with its passes, `peak - held when planned <= budget` for every stage, and the digests of the unplanned run, of the old lv1 plan under the
same budget, and of the reference's own run (tests/golden/s2_count_passes.json, tools/make_s2_count_passes_golden.py)."""
import json
import os
import re

import pytest

import golden_util as gu
from megahit_amd import canon
from test_gpu_memory_plan import PLAN_LINE, _check_budget, _core, _digests, _stages, libs  # noqa: F401  (libs: a fixture)

pytestmark = pytest.mark.gpu

COUNT_PLAN_LINE = re.compile(r"Memory plan: stage 2 from a count in (\d+) passes over its own bucket ranges")

# Where the factors c of MHX_FREE_BYTES = c * B come from (B = 20 M bases of 200 000 reads of 100; everything per base), as in
# test_gpu_memory_plan.py: plan_ranges has avail = 0.7336 * c for stage 2 (no fixed state, two staging batches of c / 32 with the allocator's
# 17/16), and one run of the route fits while 17/16 * 13 * 2.2 = 30.4 <= avail: c >= 41.4.
# Below that, mhx_s2_from_count_bytes for passes of N records (include/mhx.h; s2.hip s2_from_count_need):
#   24.5 N (two 12-byte record buffers, status words) + 1/3 (status words over all item slots) + 2 * 1.68 (the giant buckets' partial sums
#   and listed keys, 32 MiB each) + 0.08 (8 bytes per read) + 1/8 at min count 1 (the bitmap of the (k+1)-mer starts)
#   + 25 bytes per item, one item per record and 4 per read: 25 * (0.73 + 0.04) = 19.25 at k = 27, 25 * (0.75 + 0.04) = 19.75 at k = 25
#   = 24.5 N + 23.14 at (27, 1), 24.5 N + 23.52 at (25, 2); the largest N with 17/16 * that <= 0.7336 c:  N = (0.6904 c - 23.14) / 24.5
#   (27, 1), c = 39.5: N = 0.169 of 0.73 records per base: 4.3 -> 5 passes;  (25, 2), c = 40: N = (27.62 - 23.52) / 24.5 = 0.167 of 0.75: 4.5 -> 5
#   (the plan by time stays out of it: the process has allocated less than 1 GiB, so it has seen no rate)
# The old plan under the same budget (MHX_S2_AGG_FROM_COUNT=0): 0.7336 * 39.5 / 26.56 = 1.09 items a pass of the bound 2.2: lv1 passes.
# c_once = 43: a few per cent over 41.4 — one run, no plan line.
#   (k, m, c_passes, c_once)
CASES = [(27, 1, 39.5, 43), (25, 2, 40, 43)]
_unplanned = {}


def _run(libs, k, m, out, env=None):
    prefix, _, _ = libs["fixed"]
    err = _core(gu.MHX_CORE, ["read2sdbg", "-k", str(k), "-m", str(m), "--read_lib_file", prefix], out, env=env)
    return err, _digests("read2sdbg", out)


def _golden(k, m):
    with open(os.path.join(gu.GOLD, "s2_count_passes.json")) as f:
        gold = json.load(f)
    ent = [e for e in gold["cases"] if (e["k"], e["m"]) == (k, m)][0]
    return gold["library"], {key: v for key, v in ent.items() if key not in ("k", "m")}


def _unplanned_digests(libs, k, m):
    if (k, m) not in _unplanned:
        _unplanned[(k, m)] = _run(libs, k, m, os.path.join(libs["dir"], "s2cp_unplanned_k%d_m%d" % (k, m)))[1]
    return _unplanned[(k, m)]


@pytest.mark.parametrize("k,m,c_passes,c_once", CASES, ids=["k%d-m%d" % c[:2] for c in CASES])
def test_core_plans_the_count_in_passes(libs, tmp_path, k, m, c_passes, c_once):
    prefix, _, bases = libs["fixed"]
    library, gold = _golden(k, m)
    assert canon.digest_file(prefix + ".bin") == library["bin_md5"], "the library is not the one the golden file was made from"
    want = _unplanned_digests(libs, k, m)
    assert want == gold
    # the once-fit fails: 3 to 6 count passes, the new line, the budget, the digests
    err, got = _run(libs, k, m, str(tmp_path / "passes"), env=dict(MHX_FREE_BYTES=str(int(c_passes * bases))))
    print("\n".join(line for line in err.splitlines() if "Memory plan" in line or "Device memory of" in line or "plan:" in line))
    planned = COUNT_PLAN_LINE.search(err)
    assert planned and 3 <= int(planned.group(1)) <= 6, err[-2000:]
    assert "given up" not in err and "alone holds" not in err, err[-2000:]
    stages = _stages(err)
    mine = [s for s in stages if s[0] == "stage 2"]
    assert len(mine) == 1 and mine[0][4] == 1, stages  # (no lv1 plan line for stage 2)
    _check_budget(stages)
    assert got == want
    # just above the once-fit: one pass, no new line
    err, got = _run(libs, k, m, str(tmp_path / "once"), env=dict(MHX_FREE_BYTES=str(int(c_once * bases))))
    assert not COUNT_PLAN_LINE.search(err), err[-2000:]
    stages = _stages(err)
    assert [s[4] for s in stages if s[0] == "stage 2"] == [1], stages
    _check_budget(stages)
    assert got == want
    # the route switched off, or only its passes: the same budget gives the old lv1 plan
    for off in ({"MHX_S2_AGG_FROM_COUNT": "0"}, {"MHX_S2_COUNT_PASSES": "0"}):
        err, got = _run(libs, k, m, str(tmp_path / "lv1"), env=dict(off, MHX_FREE_BYTES=str(int(c_passes * bases))))
        assert not COUNT_PLAN_LINE.search(err), err[-2000:]
        stages = _stages(err)
        assert [s[4] >= 2 for s in stages if s[0] == "stage 2"] == [True], stages
        _check_budget(stages)
        assert got == want


def test_core_plans_lv1_ranges_when_the_route_gives_up(libs, tmp_path):
    """200 000 random reads of 100 bases: every (k+1)-mer is new, so the first count pass overflows its edge regions (three entries for four
    records) and the route gives up.  Under the budget of the (27, 1) case above the CLI has planned the count in passes; it reads the
    give-up from the call's message, plans lv1 ranges with the per-occurrence figure instead, stays inside its budget, and writes what the
    unplanned run writes."""
    import numpy as np
    from megahit_amd import synth
    k, m, c_passes, _ = CASES[0]
    prefix = str(tmp_path / "random")
    _, bases = synth.write_read_lib(prefix, [np.random.default_rng(7).integers(0, 4, size=(200000, 100), dtype=np.uint8)])
    args = ["read2sdbg", "-k", str(k), "-m", str(m), "--read_lib_file", prefix]
    _core(gu.MHX_CORE, args, str(tmp_path / "unplanned"))
    want = _digests("read2sdbg", str(tmp_path / "unplanned"))
    err = _core(gu.MHX_CORE, args, str(tmp_path / "planned"), env={"MHX_FREE_BYTES": str(int(c_passes * bases))})
    print("\n".join(line for line in err.splitlines() if "Memory plan" in line or "Device memory of" in line or "given up" in line))
    assert COUNT_PLAN_LINE.search(err), err[-2000:]
    assert re.search(r"stage 2 from a count given up \(an edge region overflowed in pass 1\); planning lv1 bucket ranges instead", err), err[-2000:]
    stages = _stages(err)
    assert [s[4] >= 2 for s in stages if s[0] == "stage 2"] == [True], stages
    _check_budget(stages)
    assert _digests("read2sdbg", str(tmp_path / "planned")) == want
