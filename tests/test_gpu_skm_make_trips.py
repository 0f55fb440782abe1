"""GPU: k_skm_make over SEVERAL trips per workgroup (megahit_amd/csrc/s1_skm.hip).  The kernel divides a block's number by the blocks
per read once per thread and moves quotient and remainder from block to block and from trip to trip by the steps' own quotients and
remainders with one carry; the libraries of the other test files are a few dozen trips in all, one per workgroup, so the carry from trip
to trip never runs there.  s1_skm_make_grid cuts the workgroups down: 1 (every trip in one workgroup), 4 and 7 (steps whose remainders
carry at different trips), on reads of 10 blocks (pe100), of 2 (short30: the step from a thread's first block to its second, 512, carries
twice over) and of several lengths, stage 1 and `count` — every case against the oracle exactly as test_gpu_skm_split.run does."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_skm_split import BASE, RESET as SPLIT_RESET, _oracle, run as run_split

pytestmark = pytest.mark.gpu

RESET = dict(SPLIT_RESET, s1_skm_make_grid=0)


def run(engine, key, reads, k, m, opts, **kw):
    try:
        return run_split(engine, key, reads, k, m, opts, **kw)
    finally:
        for n, v in RESET.items():
            engine.set_option(n, v)


@pytest.mark.parametrize("grid", [1, 4, 7])
@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 2), ("pe100", 19, 1), ("short30", 21, 2), ("pe100", 22, 2)])
def test_several_trips_per_workgroup(engine, kind, k, m, grid):
    seed = k * 7 + m if kind == "pe100" else k + m  # (the libraries, and the oracle's answers, of test_gpu_skm_split)
    run(engine, (kind, seed), fixed_library(kind, seed=seed), k, m, dict(BASE, s1_skm_make_grid=grid), make=1, scatter=1)


@pytest.mark.parametrize("grid", [1, 4])
@pytest.mark.parametrize("split", [1, 0])
def test_reads_of_several_lengths(engine, grid, split):
    """every read takes the blocks of the longest; the records through the ranges and through the one cursor"""
    run(engine, ("var", 11), make_reads("var", 11), 21, 2, dict(BASE, s1_var_min_fill=5, s1_skm_make_grid=grid, s1_skm_split=split), make=1, scatter=2 - split)


def test_passes_over_ranges_of_bins(engine):
    run(engine, ("pe100", 23), fixed_library("pe100", seed=23), 21, 2, dict(BASE, s1_skm_passes=3, s1_skm_make_grid=4), make=3, scatter=3)


@pytest.mark.parametrize("grid", [1, 4])
@pytest.mark.parametrize("kind", ["pe100", "var"])
def test_count_over_several_trips(engine, kind, grid):
    """`count` makes its records with the same kernel (one word of the store more per block: the base in front of it)"""
    k, m = 21, 2
    reads = make_reads(kind, 17) if kind == "var" else fixed_library(kind, seed=k * 11 + m)
    if ("count", kind, k, m) not in _oracle:
        pkg = ob.Package(reads, reverse=True)
        _oracle[("count", kind, k, m)] = (pkg, ob.count(pkg, k, m))
    pkg, want = _oracle[("count", kind, k, m)]
    load(engine, pkg)
    try:
        for n, v in dict(BASE, s1_var_min_fill=5, s1_skm_cap_pct=300, s1_skm_make_grid=grid).items():
            engine.set_option(n, v)
        engine.profile(True)
        engine.profile_reset()
        r = engine.count(k, m)
        stats = engine.profile_get()
        engine.profile(False)
        assert engine.last_s1_plan().startswith("count: super-k-mers"), engine.last_s1_plan()
        assert stats["count_skm_make"]["launches"] == 1 and stats["radix_scatter_16B"]["launches"] == 1 and "count_skm_groups" in stats
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
