"""GPU: super-k-mer records split by the low digit of their bin where they are made (s1_skm_split, megahit_amd/csrc/s1_skm.hip
k_skm_make<.., SPLIT>): the make kernel puts every record into the range of its digit, the sort starts at the second digit and reads the
ranges in order (sort_kernels.h SrcSplit), so one 16-byte pass fewer runs.  Every case against the oracle on is_solid, the multiplicity
histogram, the item count and the SdBG of stage 2 (`count`: edges, histogram, bucket counts): the split taken and not taken, a range that
overflows (the records are made again, unsplit), trips that do not fit the LDS stage, three digits and odd widths, one digit (no split),
passes over ranges of bins, reads of several lengths, position tags, `count`, several ranks, and libraries with hardly a record."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_sdbg import check_sdbg
from test_gpu_skm import RESET as SKM_RESET, repeat_reads

pytestmark = pytest.mark.gpu

RESET = dict(SKM_RESET, s1_skm_split=1, s1_skm_split_stage=2560, count_skm=1, count_skm_group=2)
BASE = dict(s1_skm=2, s1_skm_max_bin=1 << 30)

_oracle = {}


def wanted(key, reads, k, m):
    """the oracle's answers, computed once per (library, k, m)"""
    if (key, k, m) not in _oracle:
        pkg = ob.Package(reads, reverse=True)
        w1 = ob.s1(pkg, k, m, tie_stable=True)
        _oracle[(key, k, m)] = (pkg, w1, ob.s2(pkg, k, m, w1["is_solid"]))
    return _oracle[(key, k, m)]


def run(engine, key, reads, k, m, opts, make=1, scatter=1, groups=True):
    pkg, want1, want2 = wanted(key, reads, k, m)
    load(engine, pkg)
    try:
        for n, v in opts.items():
            engine.set_option(n, v)
        engine.profile(True)
        engine.profile_reset()
        r1 = engine.read2sdbg_s1(k, m)
        stats = engine.profile_get()
        engine.profile(False)
        plan = engine.last_s1_plan()
        assert plan.startswith("super-k-mers"), plan
        assert stats["s1_skm_make"]["launches"] == make, stats["s1_skm_make"]
        assert stats.get("radix_scatter_16B", {"launches": 0})["launches"] == scatter, stats.get("radix_scatter_16B")
        assert (groups is None or "s1_skm_groups" in stats) and "s1_groups" not in stats, sorted(stats)
        solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
        assert r1.n_items == want1["n_items"]
        assert np.array_equal(solid, want1["is_solid"][: solid.size])
        assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), want1["hist"])
        assert r1.n_solid == int(sum(bin(int(x)).count("1") for x in want1["is_solid"]))
        check_sdbg(engine, engine.read2sdbg_s2(k, m), want2)
        return plan
    finally:
        engine.profile(False)
        for n, v in RESET.items():
            engine.set_option(n, v)


@pytest.mark.parametrize("k,m", [(19, 1), (19, 2), (21, 1), (21, 2), (22, 1), (22, 2)])
def test_the_split_saves_one_pass(engine, k, m):
    """pe100: 474 000 windows, ~526 records per digit against ranges of 4096 slots (the array at twice its usual size): the make kernel
    runs once, ONE 16-byte pass follows it; with the knob off, two"""
    reads = fixed_library("pe100", seed=k * 7 + m)
    run(engine, ("pe100", k * 7 + m), reads, k, m, dict(BASE, s1_skm_cap_pct=72), make=1, scatter=1)
    run(engine, ("pe100", k * 7 + m), reads, k, m, dict(BASE, s1_skm_cap_pct=72, s1_skm_split=0), make=1, scatter=2)


@pytest.mark.parametrize("case", ["(AC)n", "polyA", "(AC)n, stage too small"])
def test_a_range_that_overflows_makes_the_records_again(engine, case):
    """3000 (AC)n reads put ~30 000 records behind one minimizer: its range of a few thousand slots overflows, the records are made again
    through the one cursor and ordered by all passes — the same answers, the same plan, nothing counted twice (the homopolymer windows of
    3000 poly-A reads, counted beside the records, would show in the histogram)"""
    reads = fixed_library("pe100", seed=11) + repeat_reads(3000, [0, 1])
    opts = dict(BASE)
    if case == "polyA":
        reads = reads + repeat_reads(3000, [0])
    if case.endswith("too small"):
        opts["s1_skm_split_stage"] = 64
    run(engine, ("pe100+" + case.split(",")[0], 11), reads, 21, 2, opts, make=2, scatter=2)


def test_reads_of_several_lengths_count_their_items_once(engine):
    """the item count of reads of several lengths is summed by the make kernel: a second run must start it from zero"""
    reads = make_reads("var", 11) + [r[:90] for r in repeat_reads(3000, [0, 1])]
    run(engine, ("var+(AC)n", 11), reads, 21, 2, dict(BASE, s1_var_min_fill=5), make=2, scatter=2)


@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 2), ("short30", 21, 2), ("pe100", 20, 1)])
def test_trips_that_do_not_fit_the_stage(engine, kind, k, m):
    """s1_skm_split_stage = 64: every trip writes its records from the registers to the places it reserved"""
    run(engine, (kind, k + m), fixed_library(kind, seed=k + m), k, m, dict(BASE, s1_skm_split_stage=64), make=1, scatter=1)


@pytest.mark.parametrize("bits,scatter", [(18, 2), (20, 2), (11, 1), (8, 1)])
@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 2), ("pe100", 22, 1), ("short30", 19, 1)])
def test_three_digits_odd_widths_and_one_digit(engine, kind, k, m, bits, scatter):
    """the passes behind the make kernel: one fewer than the bin has digits; a bin of ONE digit is ordered by its one pass over an array
    without holes (the group-by cannot read the ranges)"""
    run(engine, (kind, k + m), fixed_library(kind, seed=k + m), k, m, dict(BASE, s1_skm_bin_bits=bits), make=1, scatter=scatter)


@pytest.mark.parametrize("how", ["passes", "var", "tags"])
def test_passes_over_ranges_of_bins_several_lengths_and_tags(engine, how):
    k, m, opts, reads, key = 21, 2, dict(BASE), fixed_library("pe100", seed=23), ("pe100", 23)
    make = scatter = 1
    if how == "passes":  # every pass makes the records of its bins and splits them: three launches of each kernel
        opts["s1_skm_passes"] = 3
        make = scatter = 3
    if how == "var":
        reads, key = make_reads("var", 11), ("var", 11)
        opts["s1_var_min_fill"] = 5
    if how == "tags":
        opts["s1_skm_tags"] = 1
    plan = run(engine, key, reads, k, m, opts, make=make, scatter=scatter)
    if how == "passes":
        assert "3 passes over ranges of bins" in plan


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 2), ("short30", 20, 1), ("var", 21, 2)])
def test_count_on_split_records(engine, kind, k, m, split):
    """`count` makes its records with the same kernel (a base more either side): edges, histogram, bucket counts, first_0_out / last_0_in
    against the oracle's KmerCounter, the split on and off"""
    reads = make_reads(kind, 17) if kind == "var" else fixed_library(kind, seed=k * 11 + m)
    if ("count", kind, k, m) not in _oracle:
        pkg = ob.Package(reads, reverse=True)
        _oracle[("count", kind, k, m)] = (pkg, ob.count(pkg, k, m))
    pkg, want = _oracle[("count", kind, k, m)]
    load(engine, pkg)
    try:
        for n, v in dict(BASE, s1_var_min_fill=5, s1_skm_cap_pct=300, s1_skm_split=split).items():
            engine.set_option(n, v)
        engine.profile(True)
        engine.profile_reset()
        r = engine.count(k, m)
        stats = engine.profile_get()
        engine.profile(False)
        assert engine.last_s1_plan().startswith("count: super-k-mers"), engine.last_s1_plan()
        assert stats["count_skm_make"]["launches"] == 1 and stats["radix_scatter_16B"]["launches"] == 2 - split and "count_skm_groups" in stats
        assert r.n_items == want["n_items"] and r.words_per_edge == want["wpe"]
        edges = engine.fetch(lib.BUF_EDGES, np.uint32).reshape(-1, r.words_per_edge)
        assert edges.shape == want["edges"].shape and np.array_equal(edges, want["edges"])
        assert np.array_equal(engine.fetch(lib.BUF_BUCKET_COUNT, np.uint64), want["bucket_count"])
        assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), want["hist"])
        assert np.array_equal(engine.fetch(lib.BUF_FIRST_0_OUT, np.uint32), want["first_0_out"])
        assert np.array_equal(engine.fetch(lib.BUF_LAST_0_IN, np.uint32), want["last_0_in"])
    finally:
        engine.profile(False)
        for n, v in RESET.items():
            engine.set_option(n, v)


@pytest.mark.parametrize("world,k,opts", [(2, 21, {}), (3, 22, {"s1_stream_fill": 40}), (3, 21, {"s1_skm_bin_bits": 18})])
def test_several_ranks_split_their_records(world, k, opts):
    """comm.hip dist_s1_skm: every rank makes, splits and orders the records of its reads before the exchange by bin; the ranks' results
    are those of one GPU (the oracle on the union of the reads), the split on or off"""
    from test_gpu_comm import run_ranks, load_reads, all_reads, sdbg_of, check_sdbg as check_ranks

    def body(r, e, cm):
        cm.setup(0, k, 2)
        r1, r2, _ = cm.read2sdbg(k, 2)
        return sdbg_of(e) + (e.fetch(lib.BUF_MUL_HIST, np.int64), int(r1.n_solid), e.last_s1_plan(), int(r1.n_items))

    pkg = all_reads(world)
    s1 = ob.s1(pkg, k, 2)
    s2 = ob.s2(pkg, k, 2, s1["is_solid"])
    for split in (1, 0):
        outs = run_ranks(world, load_reads, body, dict(opts, s1_skm=2, s1_skm_max_bin=1 << 30, s1_var_min_fill=5, s1_skm_split=split))
        for o in outs:
            assert o[6].startswith("super-k-mers") and "exchanged by bin" in o[6], o[6]
        assert np.array_equal(sum(o[4] for o in outs), s1["hist"])
        assert sum(o[5] for o in outs) == int(sum(bin(int(x)).count("1") for x in s1["is_solid"]))
        assert sum(o[7] for o in outs) == s1["n_items"]
        check_ranks(outs, s2)


def test_a_tiny_library(engine):
    """24 reads: nearly every range is empty, and every unit of the pass still publishes its counts"""
    run(engine, ("tiny60", 5), fixed_library("tiny60", seed=5), 21, 2, dict(BASE), make=1, scatter=1)


def test_no_record_at_all(engine):
    """reads of one base only: every window is counted beside the records, every range stays empty, nothing is ordered or grouped"""
    reads = repeat_reads(300, [0]) + repeat_reads(120, [3]) + repeat_reads(50, [2], length=64)
    run(engine, ("homopolymers", 0), reads, 21, 2, dict(s1_skm=2, s1_var_min_fill=5), make=1, scatter=0, groups=None)
