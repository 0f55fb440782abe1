"""GPU: stage 2 from a count of the (k+1)-mers with the count in PASSES over its own lv1 bucket ranges (s2.hip s2_agg_from_count_passes;
options s2_count_pass_items, s2_count_budget_mb; mhx_s2_from_count_bytes) — against the oracle's per-occurrence Read2SdbgS2, against the
one-pass route and against the per-occurrence path, byte for byte: pass boundaries, empty passes, keys of huge multiplicity, the pass
cap, what the handle is left with, a give-up in a later pass, and the device bytes the route holds."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib, synth
from test_gpu_count import load
from test_gpu_memory_plan import _engine_with_reads, libs  # noqa: F401  (libs: the 200 000-read library, a fixture)
from test_gpu_round3_knobs import fixed_library
from test_gpu_sdbg import check_sdbg
from test_gpu_tile_tails import giant_library

pytestmark = pytest.mark.gpu

KERNEL = "s2_edges_to_items"
MAX_PASSES = 64  # mhx_internal.h kS2CountMaxPasses
DEFAULTS = dict(s2_count_pass_items=0, s2_count_budget_mb=0, s2_agg_from_count=1, s1_giant_min=262144)  # include/mhx.h
_wanted = {}


def several_lengths(seed):
    rng = np.random.default_rng(seed)
    return [x[: rng.integers(60, 101)] for x in synth.gen_pe_reads(2000, 5000, read_len=100, frag=250, err=0.01, seed=seed)]


def library(kind, seed):
    if kind == "var":
        return several_lengths(seed)
    if kind == "giant":
        return giant_library(seed, n_poly=1500)
    return fixed_library(kind, seed=seed)


def wanted(kind, seed, k, m):
    """-> (package, the oracle's stage 2), made once per case"""
    key = (kind, seed, k, m)
    if key not in _wanted:
        pkg = ob.Package(library(kind, seed), reverse=True)
        solid = ob.s1(pkg, k, m, tie_stable=True)["is_solid"] if m > 1 else None
        _wanted[key] = (pkg, ob.s2(pkg, k, m, solid))
    return _wanted[key]


def n_ranges(hist, cap):
    """the rule of s2_count_pass_items: contiguous ranges of lv1 buckets of at most `cap` records, a bucket above it alone in its range"""
    n, acc = 1, 0
    for v in hist.tolist():
        if acc and acc + v > cap:
            n, acc = n + 1, 0
        acc += v
    return n


def launches(stats):
    return stats[KERNEL]["launches"] if KERNEL in stats else 0


def stage2(engine, k, m, opts):
    """stage 2 (behind a new stage 1 at min count >= 2) under `opts` -> (result, SdBG bytes, profile, plan text); the options are set back"""
    before = {n: engine.get_option(n, DEFAULTS[n]) for n in opts}
    try:
        for n, v in opts.items():
            engine.set_option(n, v)
        if m > 1:
            engine.read2sdbg_s1(k, m)
        engine.profile(True)
        engine.profile_reset()
        r2 = engine.read2sdbg_s2(k, m)
        stats = engine.profile_get()
        return r2, engine.fetch(lib.BUF_SDBG_BYTES, np.uint8).copy(), stats, engine.last_s1_plan()
    finally:
        engine.profile(False)
        for n, v in before.items():
            engine.set_option(n, v)


def in_passes_equals_everything(engine, kind, seed, k, m, extra=None):
    pkg, want = wanted(kind, seed, k, m)
    load(engine, pkg)
    extra = extra or {}
    records = int(engine.bucket_histogram(lib.STAGE_COUNT, k, m).sum())
    r2, got, stats, plan = stage2(engine, k, m, dict(extra, s2_count_pass_items=records // 4))
    print("%s k=%d m=%d: %d records, %d launches of %s, plan: %s" % (kind, k, m, records, launches(stats), KERNEL, plan))
    check_sdbg(engine, r2, want)
    assert launches(stats) >= 3, sorted(stats)
    assert " passes over its own lv1 bucket ranges" in plan and "(%d records" % records in plan, plan
    r1, once, stats1, plan1 = stage2(engine, k, m, dict(extra, s2_count_pass_items=0))
    assert launches(stats1) == 1 and "passes over its own" not in plan1, (sorted(stats1), plan1)
    assert np.array_equal(got, once) and r1.n_items == r2.n_items
    _, occ, stats0, _ = stage2(engine, k, m, dict(extra, s2_agg_from_count=0))
    assert launches(stats0) == 0
    assert np.array_equal(got, occ)


@pytest.mark.parametrize("kind,k,m", [("pe100", 27, 1), ("repeats100", 27, 1), ("pe100", 21, 1), ("short30", 21, 1), ("tiny60", 21, 1), ("pe100", 23, 2),
                                      ("repeats100", 25, 3), ("var", 21, 1)])
def test_in_passes_equal_to_the_oracle(engine, kind, k, m):
    in_passes_equals_everything(engine, kind, k + m, k, m)


@pytest.mark.parametrize("k,m", [(27, 1), (27, 2), (21, 1)])
def test_multiplicities_across_passes(engine, k, m):
    """poly-A (k+1)-mers in ~10^5 records: thousands of items of one edge at k = 27 (63 per item), the 65 535 cap, palindromes ((AC)n), and
    the giant buckets cut into slices (s1_giant_min = 64) — one lv1 bucket holds half the records, so it is a pass of its own above the cap"""
    in_passes_equals_everything(engine, "giant", k + m, k, m, dict(s1_giant_min=64))


def test_pass_sizes_at_the_edges(engine):
    k, m = 27, 1
    pkg, want = wanted("giant", k + m, k, m)
    load(engine, pkg)
    hist = engine.bucket_histogram(lib.STAGE_COUNT, k, m)
    records, largest = int(hist.sum()), int(hist.max())
    rest = records - largest
    assert largest * 4 > records > largest, (records, largest)  # the poly-A bucket: at most MAX_PASSES passes of its size cover everything
    _, once, stats, _ = stage2(engine, k, m, {})
    assert launches(stats) == 1
    for size in (largest, largest - 1):  # exactly the largest bucket; one less: that bucket alone in its pass and over the cap
        r2, got, stats, plan = stage2(engine, k, m, dict(s2_count_pass_items=size))
        check_sdbg(engine, r2, want)
        assert launches(stats) == n_ranges(hist, size) >= 2 and "passes over its own" in plan, (size, sorted(stats), plan)
        assert np.array_equal(got, once)
    r2, got, stats, plan = stage2(engine, k, m, dict(s2_count_pass_items=records + 1))  # one pass
    check_sdbg(engine, r2, want)
    assert launches(stats) == 1 and "in 1 passes" in plan, plan
    assert np.array_equal(got, once)
    # more passes than the cap: the largest size, by halving, at which the rule cuts more than MAX_PASSES ranges
    size = rest
    while n_ranges(hist, size) <= MAX_PASSES:
        size //= 2
    assert size >= 1 and n_ranges(hist, 2 * size) <= MAX_PASSES
    r2, got, stats, _ = stage2(engine, k, m, dict(s2_count_pass_items=size))
    check_sdbg(engine, r2, want)
    assert launches(stats) == 0, sorted(stats)
    assert np.array_equal(got, once)


def test_the_handle_is_left_as_it_was(engine):
    k, m = 27, 1
    pkg, want = wanted("pe100", k + m, k, m)
    load(engine, pkg)
    records = int(engine.bucket_histogram(lib.STAGE_COUNT, k, m).sum())
    guarded = ("s1_stream_sub_max", "s1_stream_max3")  # what the route sets for its count at min count 1
    unset = {n: engine.get_option(n, -7) for n in guarded}
    r2, got, stats, _ = stage2(engine, k, m, dict(s2_count_pass_items=records // 4))
    assert launches(stats) >= 3
    assert {n: engine.get_option(n, -7) for n in guarded} == unset
    # no filter left: a count and a stage 1 + stage 2 on the same handle see every bucket
    wantc = ob.count(pkg, 21, 2)
    rc = engine.count(21, 2)
    assert np.array_equal(engine.fetch(lib.BUF_EDGES, np.uint32).reshape(-1, rc.words_per_edge), wantc["edges"])
    assert np.array_equal(engine.fetch(lib.BUF_BUCKET_COUNT, np.uint64), wantc["bucket_count"])
    w1 = ob.s1(pkg, 21, 2, tie_stable=True)
    r1 = engine.read2sdbg_s1(21, 2)
    assert r1.n_items == w1["n_items"]
    check_sdbg(engine, engine.read2sdbg_s2(21, 2), ob.s2(pkg, 21, 2, w1["is_solid"]))
    # a caller's filter, set before the call: the route declines as it always did (here the filter keeps every bucket)
    engine.set_bucket_filter(np.ones(lib.NUM_BUCKETS, dtype=np.uint8), expected_items=10 * records)
    try:
        r2, filtered, stats, _ = stage2(engine, k, m, dict(s2_count_pass_items=records // 4))
    finally:
        engine.set_bucket_filter(None)
    assert launches(stats) == 0, sorted(stats)
    check_sdbg(engine, r2, want)
    assert np.array_equal(filtered, got)


def test_a_give_up_in_a_later_pass(engine):
    """No knob forces it, the library does: 2 300 poly-A reads of 60 bases fill lv1 bucket 0 with one key in 75 900 records, 2 200 random
    reads of 60 make 72 600 records of as many distinct (k+1)-mers.  With passes of the size of bucket 0 the first pass is that bucket, and
    the second holds nearly only distinct keys: above 65 536 records the workgroups' edge regions hold 3 entries for 4 records
    (s1_shared.h count_record_room: 12 bytes per record for 16-byte entries), so one overflows, the pass gives up, and the per-occurrence
    path makes the same bytes without an error."""
    k, m = 27, 1
    rng = np.random.default_rng(5)
    reads = [np.zeros(60, dtype=np.uint8) for _ in range(2300)] + [rng.integers(0, 4, size=60, dtype=np.uint8) for _ in range(2200)]
    pkg = ob.Package(reads, reverse=True)
    want = ob.s2(pkg, k, 1, None)
    load(engine, pkg)
    hist = engine.bucket_histogram(lib.STAGE_COUNT, k, m)
    assert int(hist[0]) == int(hist.max()) >= 2300 * (60 - k) and 65536 < int(hist.sum()) - int(hist[0]) <= int(hist[0])
    r2, got, stats, plan = stage2(engine, k, m, dict(s2_count_pass_items=int(hist[0])))
    print("give-up: %d launches of %s, kernels %s" % (launches(stats), KERNEL, sorted(stats)))
    check_sdbg(engine, r2, want)
    assert launches(stats) == 1, sorted(stats)  # the first pass made its items, the second never got that far
    _, occ, stats0, _ = stage2(engine, k, m, dict(s2_agg_from_count=0))
    assert launches(stats0) == 0 and np.array_equal(got, occ)
    # s2_agg_from_count = 3: the same give-up fails the call with its reason, and the results of the call before it stand untouched
    with pytest.raises(lib.MhxError, match=r"stage 2 from a count given up \(an edge region overflowed in pass 2\)"):
        stage2(engine, k, m, dict(s2_count_pass_items=int(hist[0]), s2_agg_from_count=3))
    assert engine.get_option("s2_agg_from_count", 1) == 1 and engine.get_option("s2_count_pass_items", 0) == 0
    assert np.array_equal(engine.fetch(lib.BUF_SDBG_BYTES, np.uint8), occ)
    assert engine.last_s1_plan() == "stage 2 from a count in passes given up (an edge region overflowed in pass 2)"
    # and the handle serves the next job in passes
    in_passes_equals_everything(engine, "pe100", k + m, k, m)


def _growth(libs, k, m, opts):
    """stage 2 on a new handle with the 200 000 reads of 100 bases, trimmed first -> (peak - held before the call, result, bytes, launches)"""
    e = _engine_with_reads(libs, "fixed")
    try:
        for n, v in opts.items():
            e.set_option(n, v)
        e.trim()
        held, _ = e.alloc_peak(reset=True)
        e.profile(True)
        r2 = e.read2sdbg_s2(k, m)
        n = launches(e.profile_get())
        _, peak = e.alloc_peak()
        return peak - held, r2, e.fetch(lib.BUF_SDBG_BYTES, np.uint8).copy(), n
    finally:
        e.close()


def test_memory(libs):
    """The route in passes of a quarter of the records holds no more than mhx_s2_from_count_bytes says (plus the allocator's 16th) and less
    than the one-pass route.  With s2_count_budget_mb at 0.8 of the exact need (the figure asked with the items the run made as the estimate)
    it gives up.  Under s2_agg_from_count = 3 the call then fails and no per-occurrence run follows, so the peak is the route's own: at most
    the budget — it checks its need, with the 16th, before every growth of the item array — and a count pass, which runs before the first
    check.  Nothing is published, and the accumulated items are released.  Without mode 3 the per-occurrence path makes the same bytes."""
    k, m = 27, 1
    e = _engine_with_reads(libs, "fixed")
    try:
        records = int(e.bucket_histogram(lib.STAGE_COUNT, k, m).sum())
        est = int(2.2 * libs["fixed"][2])
        quarter = records // 4
        model = e.s2_from_count_bytes(k, m, est, quarter)
        model_once = e.s2_from_count_bytes(k, m, est, 0)
        count_pass = e.s2_from_count_bytes(k, m, 0, quarter)  # (no items: the count pass and the per-read scratch alone)
        assert 0 < count_pass < model < model_once
        assert e.s2_from_count_bytes(29, m, est, quarter) == 0  # the route does not apply
        grow_p, r_p, bytes_p, n_p = _growth(libs, k, m, dict(s2_count_pass_items=quarter))
        grow_1, r_1, bytes_1, n_1 = _growth(libs, k, m, {})
        print("s2 from a count: %d records; in passes of %d: peak grows %d bytes (model %d, %.3f of it), at once %d bytes (model %d); %d items"
              % (records, quarter, grow_p, model, grow_p / model, grow_1, model_once, r_p.n_items))
        assert n_p >= 3 and n_1 == 1
        assert np.array_equal(bytes_p, bytes_1)
        assert grow_p <= model * 17 / 16
        assert grow_p < grow_1
        exact = e.s2_from_count_bytes(k, m, r_p.n_items, quarter)
        budget_mb = int(0.8 * exact * 17 / 16) >> 20
        budgeted = dict(s2_count_pass_items=quarter, s2_count_budget_mb=budget_mb)
        g = lib.Engine(0)
        try:
            g.load_bin_records(np.fromfile(libs["fixed"][0] + ".bin", dtype=np.uint32), libs["fixed"][1])
            for n, v in dict(budgeted, s2_agg_from_count=3).items():
                g.set_option(n, v)
            g.trim()
            held, _ = g.alloc_peak(reset=True)
            g.profile(True)
            with pytest.raises(lib.MhxError, match="stage 2 from a count given up .*exceed s2_count_budget_mb"):
                g.read2sdbg_s2(k, m)
            n_b = launches(g.profile_get())
            held_after, peak = g.alloc_peak()
            print("budget %d MiB of an exact need of %d bytes: given up behind %d launches, peak grows %d bytes, %d held afterwards; a count pass %d"
                  % (budget_mb, exact, n_b, peak - held, held_after - held, count_pass))
            assert n_b < n_p  # before the last pass's items
            assert peak - held <= (budget_mb << 20) + count_pass * 17 / 16
            assert held_after - held <= count_pass * 17 / 16  # the accumulated items are gone
            assert g.fetch(lib.BUF_SDBG_BYTES, np.uint8).size == 0  # nothing published
            assert "given up" in g.last_s1_plan()
        finally:
            g.close()
        _, _, bytes_occ, _ = _growth(libs, k, m, dict(s2_agg_from_count=0))
        _, _, bytes_b, n_f = _growth(libs, k, m, budgeted)  # mode 1: the per-occurrence path takes over
        assert n_f == n_b
        assert np.array_equal(bytes_b, bytes_occ) and np.array_equal(bytes_b, bytes_p)
    finally:
        e.close()
