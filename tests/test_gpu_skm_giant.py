"""GPU: giant bins of the group-by on super-k-mer records in slices (s1_skm_giant; megahit_amd/csrc/skm_giant.h, s1_skm.hip k_skm_giants,
k_s1_skm<.., GIANT>, k_count_skm<.., GIANT>).  A bin of more records than one workgroup should stream — the non-periodic windows across the
edges of microsatellite stretches inside reads share the repeat's minimizer — is cut into 2^sub0 work items: item (bin, sub0, rj0) is the
rounds of the bin from (sub0, rj0) on, every item a ticket of its own in front of the batches of bins, which skip the giant ones.  Against
the oracle (is_solid, histogram, item count, the SdBG of stage 2; for count what run_count compares): the route and its plan line, every
slice count, slices that overflow and halve themselves, solid and flagged keys inside a giant bin, several giant bins, passes, the
kernels' forms, what lies beyond the feature (the cap, the work budget, a caller that planned on the path, several ranks), and the command
line."""
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import oracle_binding as ob
from megahit_amd import lib
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_skm import RESET, repeat_reads, run, run_count
from test_gpu_skm_rep import revcomp, stretch_read

pytestmark = pytest.mark.gpu

OPTS = dict(s1_skm=2, s1_skm_max_bin=1024, s1_skm_giant=1)
GIANT_RESET = dict(s1_skm_giant=0, s1_skm_giant_max=1 << 21, s1_skm_giant_keys=4096, s1_skm_giant_work_pct=25, s1_skm_giant_slices=0, s1_skm_rep=0, s1_skm_deal=2)
ANY_BUDGET = 100000000  # (s1_skm_giant_work_pct: a forced slice count is not halved to fit — it fits or the job is given up)
A, C, G, T = 0, 1, 2, 3


def go(engine, what, reads, k, m, opts, **kw):
    """one run with the new options (and s1_skm_rep, s1_skm_deal) put back afterwards: the RESET of test_gpu_skm does not know the new ones and leaves
    the dealing at form 1; -> the plan line of stage 1 / of count, taken when that call returns (at min count 1 stage 2 writes its own)"""
    name = "count" if what == "count" else "read2sdbg_s1"
    call, plans = getattr(engine, name), []

    def keeping_the_plan(*a, **kwa):
        r = call(*a, **kwa)
        plans.append(engine.last_s1_plan())
        return r

    setattr(engine, name, keeping_the_plan)
    opts = dict(dict(s1_skm_deal=2), **opts)
    try:
        if what == "count":
            if "s1_var_min_fill" in opts:
                opts = dict(opts, s1_skm_cap_pct=300)
            kw.setdefault("want_kernels", ("count_skm_make", "s1_skm_giants", "count_skm_groups"))
            run_count(engine, reads, k, m, opts, **kw)
        else:
            kw.setdefault("want_kernels", ("s1_skm_make", "s1_skm_giants", "s1_skm_groups"))
            run(engine, reads, k, m, opts, **kw)
        return plans[-1]
    finally:
        delattr(engine, name)
        for n, v in GIANT_RESET.items():
            engine.set_option(n, v)


def giants(plan):
    """-> (giant bins, slices, records of the largest) of a plan line that used slices"""
    got = re.search(r"\[(\d+) giant bins in (\d+) slices, largest (\d+) records\]", plan)
    assert got, plan
    return tuple(int(x) for x in got.groups())


def embedded(seed, n=3000, units=((A, C),), dups=False, edges=False):
    """a library plus n random reads with 40 bases of a repeat inside: the windows across the stretch's edges share the repeat's minimizer.
    dups: every tenth planted read twice, every hundredth three times; edges: of every twenty planted reads one has its stretch at offset
    1 .. 8 and one at the read's end (both among the duplicated ones) — the read's first (last) window lies in the giant bin"""
    rng = np.random.default_rng([seed, 77])
    out = fixed_library("pe100", seed)
    for i in range(n):
        at = int(rng.integers(10, 50))
        if edges and i % 20 == 0:
            at = 1 + (i // 20) % 8
        if edges and i % 20 == 10:
            at = 60
        r = stretch_read(rng, list(units[i % len(units)]), 40, at)
        out.append(r)
        if dups and i % 10 == 0:
            out.append(r.copy())
        if dups and i % 100 == 0:
            out.append(r.copy())
    return out


def whole(seed, n=3000):
    """... plus n reads that are (AC)n throughout: with s1_skm_rep = 0 one bin of 25 000 to 37 500 records at k = 21, two keys of count ~ 10^5"""
    return fixed_library("pe100", seed) + repeat_reads(n, [A, C])


# ---- 1: the route ----
def test_embedded_stretches_stay_on_the_path_in_slices(engine):
    """3000 embedded (AC) stretches, the periodic windows counted aside: the bin of the stretches' edges is worked in slices and the path
    holds; with the option off the same library is given up, as before"""
    reads = embedded(11)
    plan = go(engine, "stage 1", reads, 21, 2, dict(OPTS, s1_skm_rep=1), absent=("s1_groups",))
    n_bins, n_slices, largest = giants(plan)
    assert plan.startswith("super-k-mers") and n_bins >= 1 and n_slices >= n_bins and largest > 1024, plan
    go(engine, "stage 1", reads, 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_giant=0), want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"),
       absent=("s1_skm_groups", "s1_skm_giants"), why="super-k-mer records given up: a bin of")


def test_count_of_embedded_stretches_stays_on_the_path_in_slices(engine):
    reads = embedded(11)
    plan = go(engine, "count", reads, 21, 2, dict(OPTS, s1_skm_rep=1), absent=("count_groups",))
    n_bins, n_slices, largest = giants(plan)
    assert plan.startswith("count: super-k-mers") and n_bins >= 1 and n_slices >= n_bins and largest > 1024, plan
    go(engine, "count", reads, 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_giant=0), want_plan="count: stream", want_kernels=("count_skm_make", "count_groups"),
       absent=("count_skm_groups", "s1_skm_giants"))


# ---- 2: slice counts ----
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("slices", [1, 2, 4, 64, 1024])
@pytest.mark.parametrize("library", ["whole", "embedded"])
def test_every_slice_count(engine, library, slices, m):
    """whole (AC)n reads in the records: two keys of count ~ 10^5 and nearly every slice empty; embedded stretches: thousands of distinct keys
    of count 1, some in every slice.  (s1_skm_cap_pct: at ONE slice a single workgroup's region takes the aggregated items of the whole bin —
    the few bases beside 3000 equal stretches make some 4000 solid keys — and the regions of a job this small, cut from the spare record
    array, hold 4096 items; the larger array gives them room, as a full-size job's have)"""
    reads, rep = (whole(13), 0) if library == "whole" else (embedded(13), 1)
    plan = go(engine, "stage 1", reads, 21, m, dict(OPTS, s1_skm_rep=rep, s1_skm_giant_slices=slices, s1_skm_giant_work_pct=ANY_BUDGET, s1_skm_cap_pct=1000))
    n_bins, n_slices, largest = giants(plan)
    assert n_bins >= 1 and n_slices == n_bins * slices and largest > 1024, plan
    if library == "whole":
        assert 25000 <= largest <= 37500, plan


@pytest.mark.parametrize("slices", [1, 2, 4, 64, 1024])
@pytest.mark.parametrize("library", ["whole", "embedded"])
def test_count_every_slice_count(engine, library, slices):
    reads, rep = (whole(13), 0) if library == "whole" else (embedded(13), 1)
    plan = go(engine, "count", reads, 21, 2, dict(OPTS, s1_skm_rep=rep, s1_skm_giant_slices=slices, s1_skm_giant_work_pct=ANY_BUDGET))
    n_bins, n_slices, largest = giants(plan)
    assert n_bins >= 1 and n_slices == n_bins * slices and largest > 1024, plan


# ---- 3: a slice that overflows ----
@pytest.mark.parametrize("more", [dict(s1_stream_fill=40), dict(s1_stream_fill=3), dict(s1_stream_probes=2)], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_a_slice_that_overflows_halves_itself(engine, what, more):
    """four slices whose rounds do not fit the table: they recurse below their start (2, rj0) and stop at (2, rj0 + 1), not at (0, 1) — a
    key taken twice or not at all shows in the histogram"""
    plan = go(engine, what, embedded(17), 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_giant_slices=4, s1_skm_giant_work_pct=ANY_BUDGET, **more))
    n_bins, n_slices, _ = giants(plan)
    assert n_slices == 4 * n_bins >= 4, plan


# ---- 4: solid and flagged keys inside a giant bin ----
@pytest.mark.parametrize("what,k", [("stage 1", 19), ("stage 1", 20), ("stage 1", 21), ("stage 1", 22), ("count", 19), ("count", 20), ("count", 21)])
def test_solid_and_flagged_keys_inside_a_giant_bin(engine, what, k):
    """planted reads seen twice and three times: the aggregated items of stage 1 come from the slices; stretches at offsets 1 .. 8 and at
    the read's end, in duplicated reads: a read's first (last) window is solid without an in-edge (out-edge) — count's second expansion
    moves first_0_out / last_0_in from inside a slice"""
    reads = embedded(19 + k, dups=True, edges=True)
    for m in (2, 1):
        plan = go(engine, what, reads, k, m, dict(OPTS, s1_skm_rep=1))
        n_bins, n_slices, largest = giants(plan)
        assert n_bins >= 1 and largest > 1024, plan


# ---- 5: several giant bins ----
UNITS3 = ((A, C), (A, A, G), (A, G, A, T))


def three_units(seed):
    reads = embedded(seed, n=3600, units=UNITS3)
    planted = reads[-3600:]
    return reads + revcomp(planted[::3][:400]) + revcomp(planted[1::3][:400]) + revcomp(planted[2::3][:400])


@pytest.mark.parametrize("passes", [0, 3], ids=lambda v: "passes%d" % v)
@pytest.mark.parametrize("seed", [23, 24, 25])
@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_several_giant_bins(engine, what, seed, passes):
    """(AC), (AAG) and (AGAT) stretches and their reverse complements: a giant bin each, wherever they fall in their batches of eight bins —
    the batches skip exactly them; in passes over ranges of bins every pass plans its own"""
    plan = go(engine, what, three_units(seed), 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_passes=passes))
    n_bins, n_slices, largest = giants(plan)
    assert n_bins >= 2 and n_slices >= n_bins and largest > 1024, plan
    if passes:
        assert "%d passes over ranges of bins" % passes in plan, plan


# ---- 6: the forms of the kernels ----
@pytest.mark.parametrize("more", [dict(s1_skm_tags=1), dict(s1_skm_deal=0), dict(s1_skm_deal=1), dict(s1_skm_deal=2), dict(s1_skm_tags=1, s1_skm_deal=0)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("m", [2, 1])
def test_forms_of_stage_1(engine, more, m):
    plan = go(engine, "stage 1", embedded(29), 21, m, dict(OPTS, s1_skm_rep=1, **more))
    assert giants(plan)[0] >= 1


@pytest.mark.parametrize("more", [dict(s1_skm_tags=1), dict(count_skm_group=4), dict(s1_skm_tags=1, count_skm_group=4)], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_forms_of_count(engine, more):
    plan = go(engine, "count", embedded(29), 21, 2, dict(OPTS, s1_skm_rep=1, **more))
    assert giants(plan)[0] >= 1


@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_reads_of_several_lengths(engine, what):
    rng = np.random.default_rng(31)
    reads = make_reads("var", 21) + [stretch_read(rng, [A, C], 40, int(rng.integers(5, 50)), length=int(rng.integers(92, 121))) for _ in range(3000)]
    plan = go(engine, what, reads, 21, 2, dict(OPTS, s1_skm_rep=1, s1_var_min_fill=5))
    assert giants(plan)[0] >= 1 and "[reads of several lengths]" in plan, plan


# ---- 7: beyond the feature ----
@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_the_cap_and_the_work_budget(engine, what):
    """a bin beyond s1_skm_giant_max, and slices that would read more than s1_skm_giant_work_pct per cent of the job's records once more:
    the prefix plan does the job and its plan line says which"""
    reads = embedded(11)
    prefix = dict(want_plan="count: stream", want_kernels=("count_skm_make", "count_groups"), absent=("count_skm_groups",)) if what == "count" else \
        dict(want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"), absent=("s1_skm_groups",))
    plan = go(engine, what, reads, 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_giant_max=2000), **prefix)
    assert re.search(r"super-k-mer records given up: a bin of \d+ records, beyond s1_skm_giant_max", plan), plan
    plan = go(engine, what, reads, 21, 2, dict(OPTS, s1_skm_rep=1, s1_skm_giant_work_pct=1, s1_skm_giant_slices=1024), **prefix)
    assert re.search(r"super-k-mer records given up: a bin of \d+ records, its slices beyond s1_skm_giant_work_pct", plan), plan


def test_a_caller_that_left_the_plan_to_the_path_still_hears_when_it_gives_up(engine):
    reads = embedded(11)
    load(engine, ob.Package(reads, reverse=True))
    try:
        for n, v in dict(OPTS, s1_skm=3, s1_skm_rep=1, s1_skm_giant_max=2000).items():
            engine.set_option(n, v)
        with pytest.raises(lib.MhxError, match="super-k-mer records given up"):
            engine.read2sdbg_s1(21, 2)
    finally:
        for n, v in dict(RESET, **GIANT_RESET).items():
            engine.set_option(n, v)


def test_several_ranks_behave_as_with_the_option_off():
    """the option is for one GPU: on two ranks the stretches fill a bin as before, the ranks take the pre-sorted exchange of the prefix plan
    together, and the answer is the oracle's"""
    from test_gpu_comm import run_ranks, sdbg_of, check_sdbg as check_ranks
    world, k = 2, 21
    lib_ = embedded(11)
    reads = [lib_[r::world] for r in range(world)]

    def load_r(r, e):
        pkg = ob.Package(reads[r], reverse=True)
        e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())

    def body(r, e, cm):
        cm.setup(0, k, 2)
        cm.read2sdbg(k, 2)
        return sdbg_of(e) + (e.fetch(lib.BUF_MUL_HIST, np.int64), e.last_s1_plan())

    pkg = ob.Package(reads[0] + reads[1], reverse=True)
    s1 = ob.s1(pkg, k, 2)
    s2 = ob.s2(pkg, k, 2, s1["is_solid"])
    plans = {}
    for giant in (0, 1):
        outs = run_ranks(world, load_r, body, dict(OPTS, s1_skm_rep=1, s1_skm_giant=giant))
        for o in outs:
            assert o[5].startswith("stream") and "pre-sorted exchange" in o[5] and "super-k-mer records given up" in o[5] and "giant" not in o[5], o[5]
        assert np.array_equal(sum(o[4] for o in outs), s1["hist"])
        check_ranks(outs, s2)
        plans[giant] = [o[5] for o in outs]
    assert plans[0] == plans[1]


# ---- 8: the command line ----
@pytest.mark.parametrize("prog", ["read2sdbg", "count"])
def test_cli_reproduces_the_golden_digests(prog, tmp_path, monkeypatch):
    ent = [e for e in gu.cases() if e["case"]["prog"] == prog and e["case"]["lib"] == "r3" and e["case"]["k"] == 21 and e["case"]["m"] == 2 and
           not e["case"].get("mercy")][0]
    for name, v in dict(MHX_S1_SKM="2", MHX_S1_SKM_GIANT="1", MHX_S1_SKM_MAX_BIN="64", MHX_NUM_GPUS="1").items():
        monkeypatch.setenv(name, v)
    logs = []
    real_run = subprocess.run

    def run_keeping_stderr(args, **kw):
        kw["stderr"] = subprocess.PIPE
        p = real_run(args, **kw)
        logs.append(p.stderr.decode(errors="replace") if isinstance(p.stderr, bytes) else (p.stderr or ""))
        return p

    monkeypatch.setattr(gu.subprocess, "run", run_keeping_stderr)
    got = gu.run_case(gu.MHX_CORE, ent, str(tmp_path))
    monkeypatch.setattr(gu.subprocess, "run", real_run)
    for key, want in ent.items():
        if key not in ("case", "mercy_cand_kmsort"):  # (the digest of a file that only a run with --need_mercy writes)
            assert got.get(key) == want, key
    assert logs and "super-k-mers" in logs[-1], logs[-1][-2000:]
