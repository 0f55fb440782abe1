"""GPU: stage 1 at k = 23..27 leaves stage 2's aggregated items itself (opt-in: s1_agg_wide; s1_stream.hip k_s1_stream<WIDE>, s1.hip
S1Stage) — the compact form of stage 2 from a count: chars, flag | W, then 60 - 2k count bits, a larger multiplicity in several items —
and stage 2 sorts them where they lie (s2.hip s2_agg_in_place) instead of counting the (k+1)-mers again.  Against the oracle's
per-occurrence Read2SdbgS2 (reference src/sorting/read_to_sdbg_s2.cpp:271-440,521-614) and, byte for byte, against the same handle with
the knob off: both key widths of the table, multiplicities beyond one item's count field and beyond the 65 535 cap, palindromic
(k+1)-mers, giant buckets, tables that overflow, every way back from the bucket streaming (which leaves no items), reads of several
lengths, the shapes the knob does not touch, and a second stage 2 without a new stage 1."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_sdbg import check_sdbg
from test_gpu_tile_tails import giant_library

pytestmark = pytest.mark.gpu

MARKER = "[aggregated stage-2 items, %d count bits]"
# what a knob goes back to behind a case (megahit_amd/csrc/mhx_options.h; s1_stream_fill: 7/8 of the 8192 slots)
DEFAULTS = {"s1_giant_min": 262144, "s1_stream_fill": 7168, "s1_stream_bits": 0, "s1_stream_probes": 1024, "s1_stream_wide": 1, "s1_agg_wide": 0}
GROUP_BYS = ("count_groups", "count_giant_groups", "s1_groups", "s1_giant_groups", "s2_edges_to_items")


def count_bits(k):
    return min(16, 60 - 2 * k)


def stage2(engine, k, m):
    engine.profile(True)
    engine.profile_reset()
    try:
        r2 = engine.read2sdbg_s2(k, m)
        return r2, engine.profile_get()
    finally:
        engine.profile(False)


def run(engine, reads, k, m, opts=None, items=True, mercy=0, twice=False):
    """stage 1 + stage 2 with the knob on against the oracle; again with the knob off: the same bytes.  items: stage 1 has to leave the
    items (at k = 23..27: the marker in its plan line; no group-by and no s2_edges_to_items in stage 2) — or must not; None: either, the
    plan line says which.  -> the plan line and the kernels stage 2 launched, knob on and off"""
    pkg = ob.Package(reads, reverse=True)
    load(engine, pkg)
    opts = dict(opts or {})
    try:
        for n, v in opts.items():
            engine.set_option(n, v)
        engine.set_option("s1_agg_wide", 1)
        w1 = ob.s1(pkg, k, m, tie_stable=True)
        want = ob.s2(pkg, k, m, w1["is_solid"])
        engine.read2sdbg_s1(k, m, mercy)
        plan = engine.last_s1_plan()
        r2, stats = stage2(engine, k, m)
        print("k=%d m=%d plan: %s; stage 2 launched: %s" % (k, m, plan, sorted(stats)))
        if 23 <= k <= 27:
            if items is None:  # whichever the plan line names
                items = MARKER % count_bits(k) in plan
            assert (MARKER % count_bits(k) in plan) == items, plan
        else:  # (k <= 22 leaves its items with 16 count bits and says nothing; beyond k = 27 there are none)
            assert "[aggregated stage-2 items" not in plan, plan
        if items:
            assert not [n for n in GROUP_BYS if n in stats], sorted(stats)
        check_sdbg(engine, r2, want)
        bytes_on = engine.fetch(lib.BUF_SDBG_BYTES, np.uint8).copy()
        if twice:  # the items are consumed: the route of the knob-off run, the same bytes
            r2b, stats_b = stage2(engine, k, m)
            assert "s2_edges_to_items" in stats_b, sorted(stats_b)
            check_sdbg(engine, r2b, want)
            assert np.array_equal(engine.fetch(lib.BUF_SDBG_BYTES, np.uint8), bytes_on)
        engine.set_option("s1_agg_wide", 0)
        engine.read2sdbg_s1(k, m, mercy)
        assert "[aggregated stage-2 items" not in engine.last_s1_plan()
        r2, stats_off = stage2(engine, k, m)
        check_sdbg(engine, r2, want)
        assert np.array_equal(engine.fetch(lib.BUF_SDBG_BYTES, np.uint8), bytes_on)
        return plan, stats, stats_off
    finally:
        engine.profile(False)
        for n in list(opts) + ["s1_agg_wide"]:
            engine.set_option(n, DEFAULTS[n])


@pytest.mark.parametrize("kind", ["pe100", "repeats100"])
@pytest.mark.parametrize("k,m", [(27, 2), (23, 2), (25, 3), (26, 2)])
def test_fixed_length_parity(engine, kind, k, m):
    _, _, stats_off = run(engine, fixed_library(kind, seed=k + m), k, m)
    assert "s2_edges_to_items" in stats_off  # (with the knob off: stage 2 from a count, as before)


def test_32_bit_table_keys(engine):
    """a 19-bit prefix leaves 2 * 22 - 19 + 6 = 31 local-key bits at k = 23: the 32-bit form of the table with the compact items"""
    plan, _, _ = run(engine, fixed_library("pe100", seed=25), 23, 2, dict(s1_stream_bits=19))
    assert "stream p19" in plan, plan


@pytest.mark.parametrize("k", [27, 23])
def test_multiplicities_beyond_the_count_field_and_the_cap(engine, k):
    """~10^5 occurrences of poly-A (k+1)-mers: 63 per item at k = 27 — thousands of items of one edge —, five pieces for the 65 535 cap
    at k = 23 (14 count bits); palindromic (k+1)-mers from (AC)n"""
    run(engine, giant_library(k + 2, n_poly=1500), k, 2)


@pytest.mark.parametrize("opts", [dict(s1_giant_min=64), dict(s1_stream_fill=40)], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_with_giant_buckets_and_overflowing_tables(engine, opts):
    plan, _, _ = run(engine, fixed_library("repeats100", seed=12), 27, 2, opts)
    if "s1_giant_min" in opts:
        assert "giant buckets in slices" in plan, plan


@pytest.mark.parametrize("opts", [dict(s1_stream_probes=0), dict(s1_stream_wide=0)], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_a_way_back_leaves_no_items(engine, opts):
    """the table gives up / the segment group-by serves: no marker, stage 2 launches what it launches with the knob off (either knob
    also keeps the count of stage 2 off its bucket streaming: per-occurrence items), the same bytes"""
    _, stats, stats_off = run(engine, fixed_library("pe100", seed=7), 27, 2, opts, items=False)
    assert sorted(stats) == sorted(stats_off)
    assert {n: v["launches"] for n, v in stats.items()} == {n: v["launches"] for n, v in stats_off.items()}


def test_reads_of_several_lengths(engine):
    """stage 2 from a count refuses them (per-occurrence items with the knob off); the bucket streaming of stage 1 does not"""
    plan, stats, stats_off = run(engine, make_reads("var", 5), 27, 2, items=None)
    assert ("stream p" in plan) == (MARKER % 6 in plan), plan  # (the bucket streaming leaves the items whatever the reads' lengths)
    assert "s2_edges_to_items" not in stats_off


def test_shapes_the_knob_does_not_touch(engine):
    plan, _, _ = run(engine, fixed_library("pe100", seed=2), 21, 2)  # k <= 22: the items with 16 count bits, as before
    assert "count bits]" not in plan
    run(engine, fixed_library("pe100", seed=2), 29, 2, items=False)  # beyond the compact form
    run(engine, fixed_library("pe100", seed=2), 27, 2, items=False, mercy=1)  # mercy candidates: the classic kernel


def test_min_count_1_still_counts(engine):
    """no stage 1 at min count 1: stage 2 from a count whatever the knob says"""
    reads = fixed_library("pe100", seed=2)
    pkg = ob.Package(reads, reverse=True)
    load(engine, pkg)
    try:
        engine.set_option("s1_agg_wide", 1)
        r2, stats = stage2(engine, 27, 1)
        assert "s2_edges_to_items" in stats, sorted(stats)
        check_sdbg(engine, r2, ob.s2(pkg, 27, 1, None))
    finally:
        engine.set_option("s1_agg_wide", 0)


def test_a_second_stage_2_without_a_new_stage_1(engine):
    run(engine, fixed_library("pe100", seed=29), 27, 2, twice=True)
