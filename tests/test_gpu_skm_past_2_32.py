"""GPU: the super-k-mer paths (megahit_amd/csrc/s1_skm.hip) at read positions past 2^32.  k_skm_make splits such a position — the low 32
bits in w3, bits 32..35 in w0 >> 28 — and the TAGS forms of k_s1_skm / k_count_skm rebuild every window's position as tag + (pos < p0 ? 1 : 0):
in the dealing forms, the GIANT and LOOK forms, the count forms and the publishers of the keys counted beside the records.  A wrong carry or
a dropped tag moves a mark by exactly 2^32 to a valid address and faults nothing; the libraries of the other tests are a few MB, where every
tag is 0 (s1_skm_tags = 1 there) and no carry happens.

Here the library is the smallest that has the edge: 2^32 + a few 10^5 bases, nearly all of them poly-A reads, which the path counts beside
the records (s1_skm_hp) and whose packed words are zeros (tests/wide_pos_util.py: the sparse library B, the compact library C, and the
oracle's answer for C composed onto B; tests/test_wide_pos_model.py holds that composition to the oracle at T = 2^20).  One read S lies
across 2^32; the reads behind it hold duplicates, reads with errors, keys of count exactly 2 and 3, a giant bin of embedded (AC) stretches,
the only window of k + 1 C's and the only (ACG)n window of the job.  The TAGS form is chosen by size alone, as production reaches it.  Every
layout also runs as its twin at T = 2^20 (tag 0), against the oracle on all of B.

s1_skm = 3 and count_skm = 3, not 2: the path is as certain, and a run that gives it up raises instead of taking the prefix plan over 4.3 G
bases.

Not covered here: the exchange of super-k-mer records between ranks with non-zero tags (a rank's base is rank x stride, and several GPUs
count no homopolymer windows beside the records in stage 1: the sparse library does not reach it), and tags >= 2 outside
tests/test_gpu_fullsize_100M.py."""
import numpy as np
import pytest

import oracle_binding as ob
import wide_pos_util as wp
from megahit_amd import lib
from test_gpu_sdbg import check_sdbg
from test_gpu_skm import RESET
from test_gpu_skm_giant import GIANT_RESET, giants

pytestmark = pytest.mark.gpu

T32, T20 = 1 << 32, 1 << 20
EDGE = 1 << 22  # positions compared bit by bit at either end of the library: a mark moved by -2^32 lands near the start
BASE = dict(s1_skm=3, count_skm=3)
# s1_skm_cap_pct, records the arrays hold per 100 windows.  At 2^32: 3.7 G windows, nearly all poly-A — 1 makes two arrays of 0.6 GB, and X, S,
# X' make some 2 x 10^5 records.  The twin at 2^20: the workgroups' output regions are cut from the spare array, and the one that works the
# bin of the (AC) stretches needs more than a 256th of a small job's (as in tests/test_gpu_skm_giant.py)
BASE_T32, BASE_T20 = dict(BASE, s1_skm_cap_pct=1), dict(BASE, s1_skm_cap_pct=300)
ALL_RESET = dict(RESET, **dict(GIANT_RESET, count_skm=1, count_skm_group=2, s1_skm_max_m=2, s1_skm_split=1))
GIANT = dict(s1_skm_giant=1, s1_skm_max_bin=1024)

S1_MAIN = [(21, 2, dict()), (21, 2, dict(s1_skm_deal=0)), (21, 2, dict(s1_skm_deal=1)), (21, 2, dict(s1_skm_deal=2)), (21, 2, dict(s1_skm_bin_bits=16)),
           (21, 2, dict(s1_skm_passes=2)), (21, 2, dict(s1_skm_split=0)), (21, 2, dict(s1_stream_fill=40)), (21, 2, dict(GIANT)), (21, 2, dict(GIANT, s1_skm_rep=1)),
           (21, 2, dict(s1_skm_rep=1)), (19, 2, dict()), (22, 2, dict()), (21, 3, dict(s1_skm_max_m=4)), (21, 4, dict(s1_skm_max_m=4))]
COUNT_MAIN = [(21, 2, dict()), (21, 2, dict(count_skm_group=4)), (21, 2, dict(GIANT)), (21, 2, dict(s1_skm_rep=1)), (21, 3, dict(s1_skm_max_m=4)), (20, 1, dict())]
S1_OTHER = [(21, 2, dict()), (21, 2, dict(s1_skm_deal=0))]
COUNT_OTHER = [(21, 2, dict())]


def _cases():
    """one flat list, a library's runs in a row: a library is built and loaded when the first of its runs comes"""
    out = []
    for name in wp.LAYOUTS:
        for kind in (("random", "copy") if name == "main" else ("random",)):
            for t_at in (T20, T32):
                for what, runs in (("stage 1", S1_MAIN if name == "main" else S1_OTHER), ("count", COUNT_MAIN if name == "main" else COUNT_OTHER)):
                    out += [(name, kind, t_at, what, k, m, opts) for k, m, opts in runs]
    return out


def _id(case):
    name, kind, t_at, what, k, m, opts = case
    return "%s-%s-T%d-%s-k%d-m%d-%s" % (name, kind, t_at.bit_length() - 1, what, k, m, ",".join("%s=%d" % kv for kv in opts.items()) or "default")


class Loaded:
    """the library the engine holds, and the expectations made for it so far"""

    def __init__(self, engine):
        self.engine, self.key, self.lay, self.want, self.direct = engine, None, None, {}, None

    def use(self, name, kind, t_at, **kw):
        key = (name, kind, t_at) + tuple(sorted(kw.items()))
        if key != self.key:
            self.lay = self.direct = None  # (the 1.07 GB of the last one go first)
            self.lay = wp.build(t_at, wp.LAYOUTS[name][0], wp.LAYOUTS[name][1], 5, kind, **kw)
            self.lay.load(self.engine)
            self.key, self.want = key, {}
            if t_at == T20:
                self.direct = ob.Package(wp.b_reads(self.lay), reverse=True)
        return self.lay

    def expect(self, what, k, m):
        """T = 2^32: composed from C; the twin at 2^20: the oracle on all of B, in the same form"""
        if (what, k, m) in self.want:
            return self.want[what, k, m]
        lay = self.lay
        if self.direct is None:
            w = wp.compose_s1(lay, k, m) if what == "stage 1" else wp.compose_count(lay, k, m)
            if what == "stage 1":
                w["bits"] = lambda lo, hi, c_bits=w["c_bits"]: lay.expected_bits(c_bits, lo, hi)
            else:
                for name in ("first_0_out", "last_0_in"):
                    w[name] = lambda lo, hi, name=name, w=w: wp.expected_per_read(lay, w, name, lo, hi)
        elif what == "stage 1":
            o = ob.s1(self.direct, k, m, tie_stable=True)
            bits = wp.bits_of(o["is_solid"], lay.n_bases)
            w = dict(n_items=o["n_items"], n_solid=int(bits.sum()), hist=o["hist"], bits=lambda lo, hi: bits[lo:hi])
        else:
            w = ob.count(self.direct, k, m)
            for name in ("first_0_out", "last_0_in"):
                w[name] = lambda lo, hi, v=w[name]: v[lo:hi]
        self.want[what, k, m] = w
        return w


@pytest.fixture(scope="module")
def loaded(engine):
    held, _ = engine.alloc_peak(reset=True)
    state = Loaded(engine)
    yield state
    peak = engine.alloc_peak()[1]
    print("\npositions past 2^32: peak device bytes %d (%.2f GB), %d held before" % (peak, peak / 1e9, held))
    state.lay = state.direct = None
    tiny = ob.Package([np.zeros(64, dtype=np.uint8)], reverse=True)  # ... and nothing of the 7 GB is left for the modules behind this one
    engine.load_sequences(tiny.words(), tiny.n_seqs, 0, tiny.start())
    engine.trim()


def profiled(engine, lay, opts, call):
    """-> (result, kernels, plan line) of one call under opts; every option the module sets is put back"""
    try:
        for n, v in dict(BASE_T32 if lay.T == T32 else BASE_T20, **opts).items():
            engine.set_option(n, v)
        engine.profile(True)
        engine.profile_reset()
        r = call()
        stats = engine.profile_get()
        return r, stats, engine.last_s1_plan()
    finally:
        engine.profile(False)
        for n, v in ALL_RESET.items():
            engine.set_option(n, v)


def same_bits(engine, want, lo, hi, n_bases):
    """BUF_IS_SOLID over the words that hold base positions [lo, hi), bit by bit"""
    w_lo, w_hi = lo // 64, min((hi + 63) // 64, engine.lib.mhx_buffer_bytes(engine.h, lib.BUF_IS_SOLID) // 8)
    got = wp.bits_of(engine.fetch_range(lib.BUF_IS_SOLID, np.uint64, w_lo, w_hi - w_lo))
    p_hi = min(w_hi * 64, n_bases)
    exp = want["bits"](w_lo * 64, p_hi)
    bad = np.flatnonzero(got[: exp.size] != exp)
    assert bad.size == 0, "%d bits differ in [%d, %d): first at position %d (want %d)" % (bad.size, lo, hi, w_lo * 64 + bad[0], exp[bad[0]])
    assert not got[exp.size:].any()  # (no bit behind the last base)


def check_stage_1(engine, lay, want, k, m, opts):
    r1, stats, plan = profiled(engine, lay, opts, lambda: engine.read2sdbg_s1(k, m))
    assert plan.startswith("super-k-mers"), plan
    for kn in ("s1_skm_make", "s1_skm_groups") + (("s1_skm_giants",) if "s1_skm_giant" in opts else ()):
        assert kn in stats, sorted(stats)
    assert "s1_groups" not in stats, sorted(stats)
    if "s1_skm_giant" in opts:
        n_bins, n_slices, largest = giants(plan)
        assert n_bins >= 1 and n_slices >= n_bins and largest > 1024, plan
    if lay.T == T32 and k == 21:  # 2^17 bins by the size of the job: a third sort pass
        assert "2^%d bins" % opts.get("s1_skm_bin_bits", 17) in plan, plan
    if "s1_skm_passes" in opts:
        assert "%d passes over ranges of bins" % opts["s1_skm_passes"] in plan, plan
    print(plan, "n_items", r1.n_items, want["n_items"], "n_solid", r1.n_solid, want["n_solid"])
    assert r1.n_items == want["n_items"]
    assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), want["hist"])
    same_bits(engine, want, lay.span[0], lay.span[1], lay.n_bases)
    same_bits(engine, want, 0, min(EDGE, lay.n_bases), lay.n_bases)
    same_bits(engine, want, max(0, lay.n_bases - EDGE), lay.n_bases, lay.n_bases)
    assert r1.n_solid == want["n_solid"]
    assert wp.popcount(engine.fetch(lib.BUF_IS_SOLID, np.uint64)) == want["n_solid"]  # (the whole bitmap: wherever else a stray mark could fall)


def check_count(engine, lay, want, k, m, opts):
    r, stats, plan = profiled(engine, lay, opts, lambda: engine.count(k, m))
    assert plan.startswith("count: super-k-mers"), plan
    for kn in ("count_skm_make", "count_skm_groups") + (("s1_skm_giants",) if "s1_skm_giant" in opts else ()):
        assert kn in stats, sorted(stats)
    assert "count_groups" not in stats, sorted(stats)
    if "s1_skm_giant" in opts:
        assert giants(plan)[0] >= 1, plan
    print(plan, "n_items", r.n_items, want["n_items"])
    assert r.n_items == want["n_items"] and r.words_per_edge == want["wpe"]
    edges = engine.fetch(lib.BUF_EDGES, np.uint32).reshape(-1, r.words_per_edge)
    assert edges.shape == want["edges"].shape and np.array_equal(edges, want["edges"])
    assert np.array_equal(engine.fetch(lib.BUF_BUCKET_COUNT, np.uint64), want["bucket_count"])
    assert np.array_equal(engine.fetch(lib.BUF_MUL_HIST, np.int64), want["hist"])
    for which, name in ((lib.BUF_FIRST_0_OUT, "first_0_out"), (lib.BUF_LAST_0_IN, "last_0_in")):
        got = engine.fetch(which, np.uint32)
        assert got.size == lay.n_seqs, (name, got.size)
        step = 1 << 22  # (every read of X, S, X' exactly; every filler read the one value C's filler reads have — wp.compose_count saw to that)
        for lo in range(0, lay.n_seqs, step):
            hi = min(lay.n_seqs, lo + step)
            bad = np.flatnonzero(got[lo:hi] != want[name](lo, hi))
            assert bad.size == 0, "%s: %d reads differ, first %d" % (name, bad.size, lo + bad[0])


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_positions_past_2_32(loaded, case):
    name, kind, t_at, what, k, m, opts = case
    lay = loaded.use(name, kind, t_at)
    if t_at == T32:
        assert lay.n_bases >> 32 == 1 and lay.span[0] < T32 < lay.span[1]
    want = loaded.expect(what, k, m)
    (check_stage_1 if what == "stage 1" else check_count)(loaded.engine, lay, want, k, m, opts)


def test_stage_2_behind_stage_1(loaded):
    """stage 2 on the aggregated items stage 1 left, with enough fillers behind X' that the runs of '$' items are at the cap in C as well"""
    lay = loaded.use("main", "random", T32, f_post=33000)
    engine, k, m = loaded.engine, 21, 2
    want1 = loaded.expect("stage 1", k, m)
    want2 = ob.s2(lay.c_pkg(), k, m, want1["is_solid_c"])
    assert 2 * (len(lay.c_reads) - (lay.c_mid[1] - lay.c_mid[0])) >= 65536

    def both():
        r1 = engine.read2sdbg_s1(k, m)
        plan = engine.last_s1_plan()
        engine.profile_reset()
        return r1, plan, engine.read2sdbg_s2(k, m)

    (r1, plan1, r2), stats, _ = profiled(engine, lay, {}, both)
    assert plan1.startswith("super-k-mers"), plan1
    assert r1.n_items == want1["n_items"] and r1.n_solid == want1["n_solid"]
    print(plan1, {n: round(v["ms"], 1) for n, v in stats.items()})
    # the hand-off: 8-byte aggregated items are sorted, no item is made from the reads per occurrence
    assert "radix_scatter_8B" in stats and "s2_extract" in stats and "s2_count" not in stats, sorted(stats)
    check_sdbg(engine, r2, want2)
