"""GPU: read2sdbg (stage 1 in both record forms, the kmsort replay, add_mercy, stage 2), count and seq2sdbg with mercy edges
against the C oracle at every key, record, edge and tip-label width of 9 <= k <= 255, through the C ABI.

The inputs are wide_k_cases.library(7, k): ~200 kb with reads longer than 256 bases, every read length around k, palindromes
and hot keys.  The oracle is pinned to the reference at these widths by test_wide_k_golden_file.py and test_oracle_vs_ref.py.
Every case proves from the oracle's own output that it is not empty."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import wide_k_cases as wk
from megahit_amd import lib
from test_gpu_comm import STAGE_COUNT, run_ranks, sdbg_of
from test_gpu_comm import check_sdbg as check_ranks_sdbg
from test_gpu_count import load
from test_gpu_sdbg import check_sdbg

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=2)
def case(k):
    reads = wk.library(wk.SEED, k)
    return reads, ob.Package(reads, reverse=True)


_COUNT = {}


def oracle_count(k, m=2):
    """the oracle's count of library(SEED, k), shared between the count and the seq2sdbg tests"""
    if (k, m) not in _COUNT:
        _COUNT[(k, m)] = ob.count(case(k)[1], k, m)
    return _COUNT[(k, m)]


def popcount(bits):
    return int(np.unpackbits(np.ascontiguousarray(bits).view(np.uint8)).sum())


def check_s1(engine, r1, w1, mercy):
    assert r1.n_items == w1["n_items"]
    solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
    assert np.array_equal(solid, w1["is_solid"][: solid.size])
    assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), w1["hist"])
    assert r1.n_solid == popcount(w1["is_solid"])
    if mercy:
        assert np.array_equal(engine.fetch(lib.BUF_MERCY_CAND, np.int64), w1["mercy"])
    else:
        assert r1.n_mercy_cand == 0


def check_count(engine, r, want):
    assert r.n_items == want["n_items"]
    assert r.words_per_edge == want["wpe"]
    edges = engine.fetch(lib.BUF_EDGES, np.uint32).reshape(-1, r.words_per_edge)
    assert edges.shape == want["edges"].shape
    assert np.array_equal(edges, want["edges"])
    assert np.array_equal(engine.fetch(lib.BUF_BUCKET_COUNT, np.uint64), want["bucket_count"])
    assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), want["hist"])
    assert np.array_equal(engine.fetch(lib.BUF_FIRST_0_OUT, np.uint32), want["first_0_out"])
    assert np.array_equal(engine.fetch(lib.BUF_LAST_0_IN, np.uint32), want["last_0_in"])


@pytest.mark.parametrize("k", wk.K_ALL)
def test_read2sdbg(engine, k):
    m = 2
    reads, pkg = case(k)
    w1 = ob.s1(pkg, k, m, tie_stable=True)
    n_mercy, solid_mercy = ob.s2_add_mercy(pkg, k, w1["is_solid"], w1["mercy"])
    want, want_mercy = ob.s2(pkg, k, m, w1["is_solid"]), ob.s2(pkg, k, m, solid_mercy)
    assert w1["n_items"] > 0 and popcount(w1["is_solid"]) > 0 and int(want["bucket_tips"].sum()) > 0 and w1["mercy"].size > 0
    assert n_mercy > 0 or k < 33
    assert want["wpt"] == (k + 15) // 16
    load(engine, pkg)
    # compact records (k >= 15), no candidates; stage 2 on what stage 1 left
    check_s1(engine, engine.read2sdbg_s1(k, m, want_mercy=False), w1, False)
    check_sdbg(engine, engine.read2sdbg_s2(k, m), want)
    # key + two words per record, candidates
    check_s1(engine, engine.read2sdbg_s1(k, m, want_mercy=True), w1, True)
    assert engine.read2sdbg_add_mercy(k) == n_mercy
    solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
    assert np.array_equal(solid, solid_mercy[: solid.size])
    check_sdbg(engine, engine.read2sdbg_s2(k, m), want_mercy, per_occurrence=True)


@pytest.mark.parametrize("k", wk.K_STRIDES)
def test_read2sdbg_reference_exact_tie_order(engine, k):
    """want_mercy=2 replays kmlib::kmsort per bucket on records of 4, 6, ..., 20 words"""
    m = 2
    reads, pkg = case(k)
    w1 = ob.s1(pkg, k, m, tie_stable=False)
    assert w1["n_items"] > 0 and w1["mercy"].size > 0
    load(engine, pkg)
    r1 = engine.read2sdbg_s1(k, m, want_mercy=2)
    assert r1.n_items == w1["n_items"]
    assert np.array_equal(engine.fetch(lib.BUF_MERCY_CAND, np.int64), w1["mercy"])
    solid = engine.fetch(lib.BUF_IS_SOLID, np.uint64)
    assert np.array_equal(solid, w1["is_solid"][: solid.size])
    n_mercy, solid_mercy = ob.s2_add_mercy(pkg, k, w1["is_solid"], w1["mercy"])
    assert n_mercy > 0 or k < 33
    assert engine.read2sdbg_add_mercy(k) == n_mercy
    assert np.array_equal(engine.fetch(lib.BUF_IS_SOLID, np.uint64), solid_mercy[: solid.size])


@pytest.mark.parametrize("k", sorted(wk.K_ALL + wk.K_EDGE_WORDS))
def test_count(engine, k):
    m = 2
    reads, pkg = case(k)
    want = oracle_count(k) if k in wk.K_ALL else ob.count(pkg, k, m)
    assert want["n_items"] > 0 and want["edges"].shape[0] > 0
    assert want["wpe"] == wk.edge_words(k)
    load(engine, pkg)
    check_count(engine, engine.count(k, m), want)


def edges_package(edges, k):
    """count output -> ((k+1)-mers, multiplicities) as EdgeReader does (test_gpu_sdbg.edges_package, vectorised)"""
    j = np.arange(k + 1)
    bases = ((edges[:, j >> 4] >> (30 - 2 * (j & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    return [b for b in bases], (edges[:, -1] & 0xFFFF).astype(np.uint16)


@pytest.mark.parametrize("k", wk.K_ALL)
def test_seq2sdbg_from_edges_with_mercy(engine, k):
    reads, pkg = case(k)
    cnt = oracle_count(k)
    assert cnt["edges"].shape[0] > 0
    seqs, mult = edges_package(cnt["edges"], k)
    epkg = ob.Package(seqs, reverse=False)
    engine.load_sequences(epkg.words(), epkg.n_seqs, k + 1, None)
    engine.load_multiplicity(mult)
    want = ob.seq2sdbg(epkg, mult, k)
    assert int(want["bucket_tips"].sum()) > 0
    check_sdbg(engine, engine.seq2sdbg(k), want, per_occurrence=True)
    # mercy: candidate reads as KmerCounter::Lv0Postprocess selects them (kmer_counter.cpp:390-403)
    first, last = cnt["first_0_out"], cnt["last_0_in"]
    sel = [i for i in range(len(reads)) if first[i] != NONE and last[i] != NONE and last[i] > first[i]]
    assert sel or k < 45 or k in wk.GEN_MERCY_ZERO
    if not sel:
        return
    cand = ob.Package([reads[i][::-1] for i in sel], reverse=False)  # .cand holds the reversed reads
    n_want, mult2 = ob.gen_mercy_edges(epkg, mult, cand, k)
    assert n_want > 0 or k < 45 or k in wk.GEN_MERCY_ZERO
    engine.load_sequences(ob.Package(seqs, reverse=False).words(), len(seqs), k + 1, None)
    engine.load_multiplicity(mult)
    assert engine.gen_mercy_edges(k, cand.words(), cand.n_seqs, cand.start()) == n_want
    check_sdbg(engine, engine.seq2sdbg(k), ob.seq2sdbg(epkg, mult2, k), per_occurrence=True)


@pytest.mark.parametrize("k", [45, 63, 127, 255])
@pytest.mark.parametrize("m", [1, 3])
def test_other_min_counts(engine, k, m):
    reads, pkg = case(k)
    load(engine, pkg)
    if m == 1:  # for_sure_solid: stage 2 runs without stage 1 (main_sdbg_build.cpp:142-146)
        want = ob.s2(pkg, k, 1, None)
        assert want["n_sort_items"] > 0 and int(want["bucket_tips"].sum()) > 0
        check_sdbg(engine, engine.read2sdbg_s2(k, 1), want, per_occurrence=True)
    else:
        w1 = ob.s1(pkg, k, m, tie_stable=True)
        assert popcount(w1["is_solid"]) > 0 and w1["mercy"].size > 0
        check_s1(engine, engine.read2sdbg_s1(k, m, want_mercy=True), w1, True)
        want = ob.s2(pkg, k, m, w1["is_solid"])
        assert int(want["bucket_tips"].sum()) > 0
        check_sdbg(engine, engine.read2sdbg_s2(k, m), want)
    want = ob.count(pkg, k, m)
    assert want["edges"].shape[0] > 0
    check_count(engine, engine.count(k, m), want)


@pytest.mark.parametrize("k", [63, 127, 255])
def test_fixed_length_loading(engine, k):
    """reads of one length loaded without a start array (fixed_len): the flattened extraction path, 300-base reads"""
    m = 2
    reads = wk.fixed_library(wk.SEED, k)
    assert len(reads) > 500 and {len(r) for r in reads} == {300}
    pkg = ob.Package(reads, reverse=True)
    w1 = ob.s1(pkg, k, m, tie_stable=True)
    n_mercy, solid_mercy = ob.s2_add_mercy(pkg, k, w1["is_solid"], w1["mercy"])
    assert popcount(w1["is_solid"]) > 0 and w1["mercy"].size > 0 and n_mercy > 0
    engine.load_sequences(pkg.words(), pkg.n_seqs, 300, None)
    check_s1(engine, engine.read2sdbg_s1(k, m, want_mercy=False), w1, False)
    check_sdbg(engine, engine.read2sdbg_s2(k, m), ob.s2(pkg, k, m, w1["is_solid"]))
    check_s1(engine, engine.read2sdbg_s1(k, m, want_mercy=True), w1, True)
    assert engine.read2sdbg_add_mercy(k) == n_mercy
    want = ob.s2(pkg, k, m, solid_mercy)
    assert int(want["bucket_tips"].sum()) > 0
    check_sdbg(engine, engine.read2sdbg_s2(k, m), want, per_occurrence=True)
    want = ob.count(pkg, k, m)
    assert want["edges"].shape[0] > 0
    check_count(engine, engine.count(k, m), want)


def rank_reads(k, r):
    reads = case(k)[0]
    half = len(reads) // 2
    return reads[:half] if r == 0 else reads[half:]


def load_rank(k):
    def f(r, e):
        pkg = ob.Package(rank_reads(k, r), reverse=True)
        e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())
    return f


@pytest.mark.parametrize("k", [127, 255])
def test_read2sdbg_mercy_two_ranks(k):
    """mhx_dist_read2sdbg with mercy on two ranks (threads of this process behind the in-process transport)"""
    m = 2

    def body(r, e, cm):
        cm.setup(0, k, m)
        _r1, _r2, nm = cm.read2sdbg(k, m, need_mercy=1)
        return sdbg_of(e) + (nm,)

    outs = run_ranks(2, load_rank(k), body)
    pkg = case(k)[1]
    s1 = ob.s1(pkg, k, m, tie_stable=True)
    n_want, solid = ob.s2_add_mercy(pkg, k, s1["is_solid"], s1["mercy"])
    assert sum(o[4] for o in outs) == n_want and n_want > 0
    want = ob.s2(pkg, k, m, solid)
    assert int(want["bucket_tips"].sum()) > 0
    check_ranks_sdbg(outs, want)


@pytest.mark.parametrize("k", [127, 255])
def test_count_two_ranks(k):
    m = 2

    def body(r, e, cm):
        cm.setup(STAGE_COUNT, k, m)
        cm.count(k, m)
        return (e.fetch(lib.BUF_EDGES, np.uint32), e.fetch(lib.BUF_BUCKET_COUNT, np.uint64), e.fetch(lib.BUF_MUL_HIST, np.int64),
                e.fetch(lib.BUF_FIRST_0_OUT, np.uint32), e.fetch(lib.BUF_LAST_0_IN, np.uint32))

    outs = run_ranks(2, load_rank(k), body)
    want = oracle_count(k)
    assert want["edges"].shape[0] > 0
    assert np.array_equal(np.concatenate([o[0] for o in outs]).reshape(-1, want["wpe"]), want["edges"])
    assert np.array_equal(sum(o[1] for o in outs), want["bucket_count"])
    assert np.array_equal(sum(o[2] for o in outs), want["hist"])
    assert np.array_equal(np.concatenate([o[3] for o in outs]), want["first_0_out"])
    assert np.array_equal(np.concatenate([o[4] for o in outs]), want["last_0_in"])
