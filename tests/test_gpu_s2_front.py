"""GPU: the front of aggregated stage 2 (megahit_amd/csrc/s2.hip).  Its '$' items come from the ends of the runs of solid positions:
k_s2d_emit compacts the run ends of a workgroup's bitmap words into an LDS list and deals them one per lane (s2_dummy_list; a list
shrunk by s2_dummy_list_cap is worked off in pieces), and the digit histograms of the sort that follows are taken where the items are
made — k_agg_compact at the end of stage 1, k_s2d_emit, k_skm_hp_publish — so that the sort reads none of its own (s2_pre_hist); and the room
for the '$' items comes from a count that stage 1's pack kernel took of the run ends in the bitmap words it wrote (s2_bound_from_s1).
Every case against the oracle's SdBG: libraries with fewer bitmap words than a workgroup takes, a run end in most words, runs of one and
two positions, runs that touch word and trip boundaries, palindromic ends, every knob setting, other k, the item layouts of
s2_agg_from_count, passes over ranges of bins, the prefix plan, two ranks; which kernels ran, also behind mhx_trim; and no state left from an earlier call."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_sdbg import check_sdbg
from test_gpu_skm import RESET as SKM_RESET

pytestmark = pytest.mark.gpu

RESET = dict(SKM_RESET, s2_dummy_list=1, s2_dummy_list_cap=0, s2_pre_hist=1, s2_bound_from_s1=1, s2_agg_in_place=1, s2_agg_from_count=1, s1_pack_fixed=1)
SKM = dict(s1_skm=2, s1_skm_max_bin=1 << 30, s1_var_min_fill=5)  # stage 1 on super-k-mer records (what a full-size job takes)
PREFIX = dict(s1_skm=0)                                           # the prefix plan: the other place where aggregated items are packed
TRIP_WORDS = 256 * 8                                              # bitmap words a workgroup of k_s2d_emit takes per trip

# (s2_bound_from_s1 = 2: stage 1's count of the run ends is used AND k_s2d_bound runs: the call fails unless the two agree exactly)
SETTINGS = [dict(), dict(s2_dummy_list=0), dict(s2_dummy_list_cap=32), dict(s2_dummy_list_cap=257), dict(s2_pre_hist=0), dict(s2_bound_from_s1=0),
            dict(s2_bound_from_s1=2), dict(s2_bound_from_s1=2, s1_pack_fixed=0), dict(s2_dummy_list=0, s2_pre_hist=0, s2_bound_from_s1=0), dict(s2_agg_in_place=0)]
IDS = lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "defaults"


def rc(x):
    return (3 - x[::-1]).astype(np.uint8)


def library(kind):
    rng = np.random.default_rng(len(kind) * 131 + 7)
    if kind in ("pe100", "repeats100", "tiny60", "short30"):
        return fixed_library(kind, seed=212)
    if kind in ("var", "lowcomplex"):
        return make_reads(kind, 8)
    if kind == "k+1,k+2":  # reads of exactly 22 and 23 bases, each twice: runs of one and two positions, both ends on one bit
        r = [rng.integers(0, 4, size=22 + (i & 1), dtype=np.uint8) for i in range(700)]
        return r + [x.copy() for x in r]
    if kind == "len64":  # one read per bitmap word, every run starts on bit 0 of its word; more than two trips of a workgroup
        g = rng.integers(0, 4, size=3000, dtype=np.uint8)
        return [g[s:s + 64].copy() for s in rng.integers(0, 3000 - 64, size=2 * TRIP_WORDS + 500)]
    if kind == "word edges":
        # reads of 85 and 43 bases alternate, each pair twice: 128 bases a pair, so that at k = 21 the run of the long read fills bits 0..63
        # of its word exactly (85 - 22 = 63) and the next word begins with the 21 positions without a (k+1)-mer.  After 2200 pairs (4400
        # words: two trip boundaries where a run STARTS on the first bit of the trip) one read of 64 bases shifts everything by a word:
        # in the second half the long reads' runs END on the last bit of a trip (words 6143, 8191).
        def pairs(n):
            out = []
            for _ in range(n):
                a, b = rng.integers(0, 4, size=85, dtype=np.uint8), rng.integers(0, 4, size=43, dtype=np.uint8)
                out += [a, b, a.copy(), b.copy()]
            return out
        return pairs(1100) + [rng.integers(0, 4, size=64, dtype=np.uint8)] + pairs(1100)
    if kind == "palindromes":  # reads that begin and end with a reverse-complement palindromic 22-mer, three times each: one '$' item, not two
        out = []
        for _ in range(300):
            x, y = rng.integers(0, 4, size=11, dtype=np.uint8), rng.integers(0, 4, size=11, dtype=np.uint8)
            read = np.concatenate([x, rc(x), rng.integers(0, 4, size=56, dtype=np.uint8), y, rc(y)])
            out += [read, read.copy(), read.copy()]
        return out + fixed_library("pe100", seed=5)[:2000]
    raise ValueError(kind)


LIBRARIES = ["pe100", "repeats100", "tiny60", "short30", "var", "lowcomplex", "k+1,k+2", "len64", "word edges", "palindromes"]
_oracle = {}


def wanted(kind, k, m):
    """the library and the oracle's answers, computed once per (library, k, m)"""
    if (kind, k, m) not in _oracle:
        pkg = ob.Package(library(kind), reverse=True)
        w1 = ob.s1(pkg, k, m, tie_stable=True) if m > 1 else None
        _oracle[(kind, k, m)] = (pkg, w1, ob.s2(pkg, k, m, w1["is_solid"] if w1 else None))
    return _oracle[(kind, k, m)]


def both_stages(engine, kind, k, m, opts, stage2_twice=False, reload=True, trim=False):
    """stage 1 and stage 2 under opts; -> (the kernels of stage 2, stage 1's plan).  reload=False: on the library the engine holds
    (loading clears what an earlier stage 1 left in the handle).  trim: the workspaces are released between the stages"""
    pkg, want1, want2 = wanted(kind, k, m)
    if reload:
        load(engine, pkg)
    try:
        for n, v in opts.items():
            engine.set_option(n, v)
        if m > 1:
            r1 = engine.read2sdbg_s1(k, m)
            assert r1.n_items == want1["n_items"]
            solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
            assert np.array_equal(solid, want1["is_solid"][: solid.size])
        plan = engine.last_s1_plan()
        if trim:
            engine.trim()
        engine.profile(True)
        engine.profile_reset()
        r2 = engine.read2sdbg_s2(k, m)
        stats = engine.profile_get()
        engine.profile(False)
        check_sdbg(engine, r2, want2)
        if stage2_twice:  # the sort consumed the aggregated items: the second call makes its items per occurrence
            check_sdbg(engine, engine.read2sdbg_s2(k, m), want2, per_occurrence=True)
        return stats, plan
    finally:
        engine.profile(False)
        for n, v in RESET.items():
            engine.set_option(n, v)


def launches(stats, name):
    return stats.get(name, {"launches": 0})["launches"]


def test_the_libraries_have_the_shapes_they_are_named_for():
    k = 21
    _, w1, _ = wanted("word edges", k, 2)
    words = w1["is_solid"]
    first_bit = [w for w in range(TRIP_WORDS, words.size, TRIP_WORDS) if int(words[w]) & 1 and not int(words[w - 1]) >> 63]
    last_bit = [w for w in range(TRIP_WORDS - 1, words.size - 1, TRIP_WORDS) if int(words[w]) >> 63 and not int(words[w + 1]) & 1]
    assert first_bit and last_bit, (first_bit, last_bit)  # a run starts on the first bit of a trip; another ends on the last bit of one
    assert words.size > 4 * TRIP_WORDS
    assert wanted("len64", k, 2)[1]["is_solid"].size > 2 * TRIP_WORDS
    assert wanted("tiny60", k, 2)[1]["is_solid"].size < 256
    _, w1, _ = wanted("short30", k, 2)
    with_end = sum(1 for w in w1["is_solid"] if int(w) & ~(int(w) << 1) & (2 ** 64 - 1))
    assert with_end * 2 > w1["is_solid"].size
    pkg, w1, _ = wanted("palindromes", k, 2)
    start = pkg.start()
    for r in range(0, 900, 3):  # the first and the last (k+1)-mer of these reads are solid: the run ends are the palindromes
        for p in (int(start[r]), int(start[r + 1]) - k - 1):
            assert (int(w1["is_solid"][p >> 6]) >> (p & 63)) & 1


@pytest.mark.parametrize("opts", SETTINGS, ids=IDS)
@pytest.mark.parametrize("plan", [SKM, PREFIX], ids=["skm", "prefix"])
@pytest.mark.parametrize("kind", LIBRARIES)
def test_every_library_under_every_setting(engine, kind, plan, opts):
    both_stages(engine, kind, 21, 2, dict(plan, **opts))


@pytest.mark.parametrize("opts", [dict(), dict(s2_dummy_list_cap=257, s2_bound_from_s1=2), dict(s2_dummy_list=0, s2_pre_hist=0, s2_bound_from_s1=0)], ids=IDS)
@pytest.mark.parametrize("kind,k,m", [("pe100", 22, 2), ("repeats100", 22, 2), ("pe100", 19, 2), ("word edges", 19, 2), ("var", 15, 2), ("lowcomplex", 15, 2)])
def test_other_k(engine, kind, k, m, opts):
    both_stages(engine, kind, k, m, dict(SKM, **opts))


@pytest.mark.parametrize("opts", [dict(), dict(s2_dummy_list_cap=32, s2_bound_from_s1=2), dict(s2_dummy_list=0)], ids=IDS)
@pytest.mark.parametrize("kind,k,m", [("pe100", 27, 1), ("pe100", 23, 2), ("repeats100", 23, 2), ("repeats100", 27, 1)])
def test_items_from_a_count_with_their_own_layout(engine, kind, k, m, opts):
    """s2_agg_from_count: count bits of 60 - 2k, flag and W right above them (other fsh / bsh / csh in k_s2d_emit)"""
    stats, _ = both_stages(engine, kind, k, m, opts)
    assert "s2_edges_to_items" in stats and launches(stats, "s2_extract") == 1, sorted(stats)


@pytest.mark.parametrize("plan", [SKM, PREFIX], ids=["skm", "prefix"])
def test_which_kernels_ran(engine, plan):
    """at the defaults the sort of stage 2 reads no histogram: the producers of its items took them; with a knob at 0 it is back"""
    stats, text = both_stages(engine, "pe100", 21, 2, dict(plan))
    assert text.startswith("super-k-mers") == (plan is SKM), text
    assert "radix_hist_all_8B" not in stats and "s2_bound" not in stats, sorted(stats)
    assert launches(stats, "s2_extract") == 1 and launches(stats, "radix_scatter_8B") == 6, stats
    for off in (dict(s2_pre_hist=0), dict(s2_dummy_list=0)):
        stats, _ = both_stages(engine, "pe100", 21, 2, dict(plan, **off))
        assert launches(stats, "radix_hist_all_8B") == 1 and "s2_bound" not in stats, (off, sorted(stats))
        assert launches(stats, "s2_extract") == 1 and launches(stats, "radix_scatter_8B") == 6, stats
    stats, _ = both_stages(engine, "pe100", 21, 2, dict(plan, s2_bound_from_s1=0))
    assert launches(stats, "s2_bound") == 1 and "radix_hist_all_8B" not in stats, sorted(stats)
    assert launches(stats, "s2_extract") == 1 and launches(stats, "radix_scatter_8B") == 6, stats


@pytest.mark.parametrize("opts", [dict(), dict(s2_dummy_list_cap=257, s2_bound_from_s1=2)], ids=IDS)
def test_items_appended_pass_by_pass(engine, opts):
    """s1_skm_passes = 3: every pass packs its items behind the earlier ones and adds to the same histograms (the front of the next pass
    writes the sort's own workspace in between); the homopolymer keys' items come last"""
    reads_key = "repeats100"
    stats, plan = both_stages(engine, reads_key, 21, 2, dict(SKM, s1_skm_passes=3, **opts))
    assert "3 passes over ranges of bins" in plan, plan
    assert "radix_hist_all_8B" not in stats, sorted(stats)


def test_stage_2_twice_after_one_stage_1(engine):
    both_stages(engine, "pe100", 21, 2, dict(SKM), stage2_twice=True)
    both_stages(engine, "short30", 21, 2, dict(PREFIX), stage2_twice=True)


# stage 2's launches behind a trim, as the commit before the hand-off record (csrc/s1_handoff.h) made them.  tiny60: 24 random reads share
# no (k+1)-mer — no solid position, no item, nothing to emit or sort; and the prefix plan marks the SOLID occurrences of a job this small
# (no sample of the polarity under 2^16 items), so its pack kernel counts no run ends and k_s2d_bound runs
NOTHING = {"s2_extract": 0, "s2_bound": 0, "radix_hist_all_8B": 0, "radix_scatter_8B": 0}
TRIMMED = {("tiny60", "skm"): NOTHING, ("tiny60", "prefix"): dict(NOTHING, s2_bound=1),
           ("pe100", "skm"): {"s2_extract": 1, "s2_bound": 0, "radix_hist_all_8B": 1, "radix_scatter_8B": 6},
           ("pe100", "prefix"): {"s2_extract": 1, "s2_bound": 0, "radix_hist_all_8B": 1, "radix_scatter_8B": 6}}


@pytest.mark.parametrize("plan", ["skm", "prefix"])
@pytest.mark.parametrize("kind", ["tiny60", "pe100"])
def test_workspaces_trimmed_between_the_stages(engine, kind, plan):
    """mhx_trim between stage 1 and stage 2: the aggregated items stay, the rows of their histograms go with ws "s2_pre_hist" (the sort
    takes its histograms itself), the bound of the '$' items lives in the handle and the bitmap is a result (no k_s2d_bound)"""
    stats, _ = both_stages(engine, kind, 21, 2, dict(SKM if plan == "skm" else PREFIX), trim=True)
    got = {n: launches(stats, n) for n in NOTHING}
    print(kind, plan, got)
    assert got == TRIMMED[kind, plan], (got, sorted(stats))


@pytest.mark.parametrize("bound", [1, 2], ids=["bound from stage 1", "bound cross-checked"])
@pytest.mark.parametrize("plan", [SKM, PREFIX], ids=["skm", "prefix"])
def test_nothing_is_left_from_an_earlier_stage_1(engine, plan, bound):
    """stage 1 at (21, 2), stage 1 at (22, 2), stage 2, all on ONE loaded library (loading would clear the handle's state): the records of
    (22, 2) — no histogram and no bound of the first call's items.  (19, 2) in front as well: fewer sort passes, another plan signature."""
    pkg, _, _ = wanted("pe100", 21, 2)
    wanted("pe100", 22, 2)
    load(engine, pkg)
    try:
        for n, v in plan.items():
            engine.set_option(n, v)
        engine.read2sdbg_s1(19, 2)
        engine.read2sdbg_s1(21, 2)
    finally:
        for n, v in RESET.items():
            engine.set_option(n, v)
    stats, _ = both_stages(engine, "pe100", 22, 2, dict(plan, s2_bound_from_s1=bound), reload=False)
    assert "radix_hist_all_8B" not in stats and ("s2_bound" in stats) == (bound == 2), sorted(stats)
    # ... and back: stage 1 at (21, 2) on the same handle, after a stage 2 has consumed the items of (22, 2)
    stats, _ = both_stages(engine, "pe100", 21, 2, dict(plan, s2_bound_from_s1=bound), reload=False)
    assert "radix_hist_all_8B" not in stats and ("s2_bound" in stats) == (bound == 2), sorted(stats)


def test_a_bitmap_set_by_the_caller(engine):
    """the caller's bitmap replaces stage 1's: stage 2 makes every item per occurrence, and nothing of stage 1's items is used"""
    pkg, want1, want2 = wanted("pe100", 21, 2)
    load(engine, pkg)
    engine.read2sdbg_s1(21, 2)
    engine.set_is_solid(want1["is_solid"])
    check_sdbg(engine, engine.read2sdbg_s2(21, 2), want2, per_occurrence=True)


def test_mercy_edges_change_the_bitmap(engine):
    """stage 1 with mercy candidates, the mercy edges added: stage 2 counts the run ends of the bitmap as it is now"""
    pkg = ob.Package(library("pe100"), reverse=True)
    load(engine, pkg)
    k, m = 21, 2
    w1 = ob.s1(pkg, k, m, tie_stable=True)
    n_want, solid_want = ob.s2_add_mercy(pkg, k, w1["is_solid"], w1["mercy"])
    engine.read2sdbg_s1(k, m, want_mercy=True)
    assert engine.read2sdbg_add_mercy(k) == n_want
    solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
    assert np.array_equal(solid, solid_want[: solid.size])
    engine.set_option("s2_bound_from_s1", 2)
    try:
        check_sdbg(engine, engine.read2sdbg_s2(k, m), ob.s2(pkg, k, m, solid_want), per_occurrence=True)
    finally:
        engine.set_option("s2_bound_from_s1", 1)


@pytest.mark.parametrize("opts", [dict(), dict(s2_dummy_list_cap=32), dict(s2_dummy_list=0)], ids=IDS)
def test_two_ranks(opts):
    """the '$' items of a rank come from the bitmap of its local reads (global_bases set)"""
    from test_gpu_comm import run_ranks, load_reads, all_reads, sdbg_of, check_sdbg as check_ranks

    def body(r, e, cm):
        cm.setup(0, 21, 2)
        cm.read2sdbg(21, 2)
        return sdbg_of(e)

    if "ranks" not in _oracle:
        pkg = all_reads(2)
        s1 = ob.s1(pkg, 21, 2)
        _oracle["ranks"] = ob.s2(pkg, 21, 2, s1["is_solid"])
    check_ranks(run_ranks(2, load_reads, body, dict(opts)), _oracle["ranks"])
