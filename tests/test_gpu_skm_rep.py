"""GPU: short tandem repeats counted beside the super-k-mer records (s1_skm_rep; megahit_amd/csrc/s1_skm.hip k_skm_make<.., REP>,
k_skm_rep_publish, k_count_rep_publish).  A (k+1)-mer of period <= 4 is its first four (or three) bases repeated: such windows never
enter a record — all windows of an (AC)n stretch share one minimizer and would fill one bin — but are tallied per entry of a table of 320
while the records are made and turned into keys behind the group-by's last pass.  Against the oracle (is_solid, histogram, item count,
the SdBG of stage 2; for count what run_count compares): every kind of unit at k + 1 even and odd, a unit and its reverse complement,
exact small counts with their marks, block and read edges, several lengths, passes and trips, libraries of repeats only, what lies beyond
the feature (period 5, s1_skm_hp = 0, several ranks), embedded stretches, seeded random libraries, and the command line."""
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
import oracle_binding as ob
from test_gpu_count import make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_skm import repeat_reads, run, run_count

pytestmark = pytest.mark.gpu

OPTS = dict(s1_skm=2, s1_skm_max_bin=1024, s1_skm_rep=1)
S1_KERNELS = ("s1_skm_make", "s1_skm_groups", "s1_skm_rep")
COUNT_KERNELS = ("count_skm_make", "count_skm_groups", "count_skm_rep")
A, C, G, T = 0, 1, 2, 3
UNITS = {"AC": [A, C], "AT": [A, T], "CG": [C, G], "AG": [A, G], "AAG": [A, A, G], "ACG": [A, C, G], "ACGT": [A, C, G, T], "AGAT": [A, G, A, T],
         "AAAC": [A, A, A, C]}


def go(engine, what, reads, k, m, opts, **kw):
    """one run with the option put back afterwards (the RESET of test_gpu_skm does not know it); -> the plan line of stage 1 / of count
    (taken when that call returns: at min count 1 stage 2 writes a plan line of its own)"""
    name = "count" if what == "count" else "read2sdbg_s1"
    call, plans = getattr(engine, name), []

    def keeping_the_plan(*a, **kwa):
        r = call(*a, **kwa)
        plans.append(engine.last_s1_plan())
        return r

    setattr(engine, name, keeping_the_plan)
    try:
        if what == "count":
            if "s1_var_min_fill" in opts:
                opts = dict(opts, s1_skm_cap_pct=300)
            kw.setdefault("want_kernels", COUNT_KERNELS)
            run_count(engine, reads, k, m, opts, **kw)
        else:
            kw.setdefault("want_kernels", S1_KERNELS)
            run(engine, reads, k, m, opts, **kw)
        return plans[-1]
    finally:
        delattr(engine, name)
        engine.set_option("s1_skm_rep", 0)


def beside(plan):
    got = re.search(r"\[(\d+) windows of period <= 4 beside the records\]", plan)
    assert got, plan
    return int(got.group(1))


def periodic_windows(reads, k):
    """the (k+1)-mers of period 3 or 4 (periods 1 and 2 are periods 4) in the reads"""
    n = 0
    for r in reads:
        r = np.asarray(r)
        if len(r) < k + 1:
            continue
        hit = np.zeros(len(r) - k, dtype=bool)
        for p in (3, 4):
            ne = np.concatenate([[0], np.cumsum(r[p:] != r[:-p])])  # window w: no unequal pair among w .. w + k - p
            w = np.arange(len(r) - k)
            hit |= ne[w + k + 1 - p] == ne[w]
        n += int(hit.sum())
    return n


def rolled(n, unit, length=100):
    """n reads that are the unit repeated from end to end, at rotating phases"""
    return [np.tile(np.roll(np.array(unit, dtype=np.uint8), i % len(unit)), length // len(unit) + 1)[:length] for i in range(n)]


def revcomp(reads):
    return [(3 - np.asarray(r)[::-1]).astype(np.uint8) for r in reads]


def stretch_read(rng, unit, n, at, length=100):
    """a random read with exactly n bases of the repeat from `at` on and a period-breaking base either side"""
    r = rng.integers(0, 4, size=length, dtype=np.uint8)
    rep = np.tile(np.array(unit, dtype=np.uint8), n)[:n]
    r[at:at + n] = rep
    p = len(unit)
    if at > 0:
        r[at - 1] = (int(rep[p - 1]) + 1) % 4  # (the base the repeat would have there is rep[p - 1])
    if at + n < length:
        r[at + n] = (int(rep[n - p]) + 1) % 4
    return r


def case_library(case, seed):
    base = fixed_library("pe100", seed)
    if case == "route":
        return base + repeat_reads(3000, [A, C]), {}
    if case == "var":
        return make_reads("var", 21) + repeat_reads(500, [A, C], length=77) + repeat_reads(300, [A, A, G], length=33), dict(s1_var_min_fill=5)
    if case == "passes":
        return base + repeat_reads(3000, [A, C]), dict(s1_skm_passes=3)
    if case == "trips":
        return base + repeat_reads(3000, [A, C]), dict(s1_skm_make_grid=2)
    if case == "only":
        return repeat_reads(300, [A, C]) + repeat_reads(120, [A, A, G]) + repeat_reads(50, [G, T], length=64), dict(s1_var_min_fill=5)
    raise ValueError(case)


# ---- 1: the route ----
def test_repeat_reads_stay_on_the_path(engine):
    """3000 (AC)n reads beside a library: with the option their windows are counted aside — as many as numpy finds — and the path holds;
    the key's count is far above the histogram's last bin.  Without the option the same library is given up, as before"""
    reads, _ = case_library("route", 11)
    plan = go(engine, "stage 1", reads, 21, 2, OPTS)
    assert beside(plan) == periodic_windows(reads, 21) >= 3000 * 79
    assert ob.s1(ob.Package(reads, reverse=True), 21, 2, tie_stable=True)["hist"][-1] >= 1
    go(engine, "stage 1", reads, 21, 2, dict(OPTS, s1_skm_rep=0), want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"), absent=("s1_skm_groups", "s1_skm_rep"),
       why="super-k-mer records given up: a bin of")


# ---- 2: every kind of unit ----
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("k", [19, 20, 21, 22])
@pytest.mark.parametrize("kind", sorted(UNITS) + ["AC+GT", "AC+polyA+polyG"])
def test_every_kind_of_unit(engine, kind, k, m):
    """period 2, 3 and 4 at every phase; AT and CG are their own reverse complement at k + 1 even, ACGT a rotation of its own; 700 reads of
    AC and 200 of GT merge into one key per rotation; homopolymer windows go the same way with the option on"""
    reads = fixed_library("pe100", k * 3 + m)
    if kind == "AC+GT":
        reads = reads + rolled(700, [A, C]) + rolled(200, [G, T])
    elif kind == "AC+polyA+polyG":
        reads = reads + rolled(3000, [A, C]) + repeat_reads(500, [A]) + repeat_reads(200, [G]) + repeat_reads(90, [T])
    else:
        reads = reads + rolled(3000, UNITS[kind])
    plan = go(engine, "stage 1", reads, k, m, OPTS)
    assert beside(plan) == periodic_windows(reads, k)


# ---- 3: exact small counts ----
@pytest.mark.parametrize("case", ["one window", "two keys", "twice", "one window, tags"])
def test_exact_small_counts(engine, case):
    """exactly k + 1 bases of (AC) in a random read: one window of count 1, marked at its position; k + 2 bases: two keys of count 1; the
    read twice: count 2, solid, aggregated items"""
    k, m, opts = 21, 2, dict(OPTS)
    rng = np.random.default_rng(4)
    r = stretch_read(rng, [A, C], k + 2 if case == "two keys" else k + 1, 30)
    reads = fixed_library("pe100", 13) + [r] + ([r.copy()] if case == "twice" else [])
    if case == "one window, tags":
        opts["s1_skm_tags"] = 1
    plan = go(engine, "stage 1", reads, k, m, opts)
    assert beside(plan) == periodic_windows(reads, k) >= (2 if case in ("two keys", "twice") else 1)


# ---- 4: block and read edges ----
WHAT_K = [("stage 1", 21), ("count", 19), ("count", 20), ("count", 21)]  # count: k + 1 even and odd, as its cases 1 to 6 ask


@pytest.mark.parametrize("what,k", WHAT_K)
def test_a_stretch_at_every_slot_of_a_block(engine, what, k):
    """k + 4 bases of (AC) from every offset 0 .. 16 of a read (every slot of a block of 8 windows, and across two blocks), one that ends
    at the read's last base, and the same reads once more: counts 1 and 2"""
    rng = np.random.default_rng(9)
    extra = [stretch_read(rng, [A, C], k + 4, at) for at in range(17)] + [stretch_read(rng, [A, C], k + 4, 100 - (k + 4))]
    for m, reads in ((2, extra), (1, extra), (2, extra + [r.copy() for r in extra[1:17]])):
        reads = fixed_library("pe100", 15) + reads
        plan = go(engine, what, reads, k, m, OPTS)
        assert beside(plan) == periodic_windows(reads, k)


@pytest.mark.parametrize("what,k", WHAT_K)
def test_reads_that_are_one_repeat_and_barely_longer_than_a_window(engine, what, k):
    """reads of k + 1, k + 8 and k + 9 bases that are (AC)n or (AAG)n throughout: one window, a full block, a block and one window"""
    reads = make_reads("var", 21)
    for n in (k + 1, k + 8, k + 9):
        reads = reads + rolled(40, [A, C], length=n) + rolled(9, [A, A, G], length=n)
    plan = go(engine, what, reads, k, 2, dict(OPTS, s1_var_min_fill=5))
    assert beside(plan) == periodic_windows(reads, k)


# ---- 5, 6: several lengths, passes, trips; repeats only ----
@pytest.mark.parametrize("case", ["var", "passes", "trips", "only"])
def test_lengths_passes_trips_and_repeats_only(engine, case):
    """windows are counted once, not once per pass over a range of bins; a workgroup of several trips adds its tallies up before it
    flushes them; a library of repeats only makes no record at all"""
    reads, more = case_library(case, 11)
    plan = go(engine, "stage 1", reads, 21, 2, dict(OPTS, **more), **(dict(want_kernels=("s1_skm_make", "s1_skm_rep")) if case == "only" else {}))
    assert beside(plan) == periodic_windows(reads, 21)
    if case == "only":
        assert "(0 records" in plan, plan


# ---- more entries in one workgroup than its LDS hash has slots ----
MANY_UNITS = [[A, C], [A, A, G], [A, G, A, T], [A, A, A, C], [A, C, G], [A, A, T], [A, C, C], [A, A, A, G], [A, A, C, G], [A, C, G, T], [A, T], [C, G]]


@pytest.mark.parametrize("slots", [64, 3, 0], ids=lambda v: "slots%d" % v)
@pytest.mark.parametrize("what,k", WHAT_K)
def test_more_entries_than_the_workgroups_hash_holds(engine, what, k, slots):
    """ONE workgroup makes all records (s1_skm_make_grid = 1) of a library with reads of twelve units at every phase and on both strands: 68
    entries where the hash of a workgroup has 48 slots (count: 16), so the entries that find none are tallied in the global table from the
    registers, the lanes of a wavefront with the same entry adding once between them (stage 1: count and smallest position; count: the nine
    tallies).  s1_skm_rep_slots = 3: nearly all entries go that way; 0: all of them — and with them the library's last reads, which hold
    exactly k + 1 bases of (CT), one window of a key seen once whose mark then comes from the global table's position, and k + 1 bases of
    (CCG) twice: a solid key from it"""
    rng = np.random.default_rng(31)
    base = fixed_library("pe100", 29)
    planted, entries = [], set()
    for unit in MANY_UNITS:
        new = rolled(60, unit)
        new = new + revcomp(new[:24])
        planted += new
        entries |= {tuple(r[:3 if len(unit) == 3 else 4]) for r in new}  # (reads that are one repeat: an entry per distinct start)
    assert len(entries) == 68
    once, twice = stretch_read(rng, [C, T], k + 1, 30), stretch_read(rng, [C, C, G], k + 1, 41)
    reads = base + planted + rolled(110, [A, A, A, C]) + [once, twice, twice.copy()]
    for m in (2, 1):
        try:
            plan = go(engine, what, reads, k, m, dict(OPTS, s1_skm_make_grid=1, s1_skm_rep_slots=slots))
        finally:
            engine.set_option("s1_skm_rep_slots", 64)
        assert beside(plan) == periodic_windows(reads, k)


# ---- 7: beyond the feature ----
def test_period_five_and_the_homopolymer_switch(engine):
    """3000 (ACGTT)n reads are given up as today; 20 stay in the records; with s1_skm_hp = 0 the option is not looked at"""
    base = fixed_library("pe100", 11)
    go(engine, "stage 1", base + rolled(3000, [A, C, G, T, T]), 21, 2, OPTS, want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"), absent=("s1_skm_groups",),
       why="super-k-mer records given up: a bin of")
    plan = go(engine, "stage 1", base + rolled(20, [A, C, G, T, T]), 21, 2, OPTS)
    assert beside(plan) == periodic_windows(base, 21)
    go(engine, "stage 1", base + repeat_reads(3000, [A, C]), 21, 2, dict(OPTS, s1_skm_hp=0), want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"),
       absent=("s1_skm_groups", "s1_skm_rep", "s1_skm_hp"), why="super-k-mer records given up: a bin of")


# ---- 8: embedded stretches ----
@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_embedded_stretches(engine, what):
    """twelve random reads with 40 bases of (AC) in the middle: at most 12 x 20 of their non-periodic windows share the repeat's minimizer,
    so one bin gains at most 240 records and the limit of 1024 holds"""
    rng = np.random.default_rng(21)
    reads = fixed_library("pe100", 19) + [stretch_read(rng, [A, C], 40, 30) for _ in range(12)]
    plan = go(engine, what, reads, 21, 2, OPTS)
    assert beside(plan) == periodic_windows(reads, 21) >= 12 * (40 - 21)


# ---- 9: count ----
@pytest.mark.parametrize("k", [19, 20, 21])
@pytest.mark.parametrize("case", ["route", "var", "passes", "trips", "only"])
def test_count_cases(engine, case, k):
    reads, more = case_library(case, 17)
    plan = go(engine, "count", reads, k, 2, dict(OPTS, **more), **(dict(want_kernels=("count_skm_make", "count_skm_rep")) if case == "only" else {}))
    assert beside(plan) == periodic_windows(reads, k)
    if case == "route" and k == 21:
        go(engine, "count", reads, k, 2, dict(OPTS, s1_skm_rep=0), want_plan="count: stream", want_kernels=("count_skm_make", "count_groups"),
           absent=("count_skm_groups", "count_skm_rep"))


@pytest.mark.parametrize("k", [19, 20, 21])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("kind", sorted(UNITS) + ["AC+GT", "AC+polyA+polyG"])
def test_count_every_kind_of_unit(engine, kind, k, m):
    reads = fixed_library("pe100", k * 5 + m)
    if kind == "AC+GT":
        reads = reads + rolled(700, [A, C]) + rolled(200, [G, T])
    elif kind == "AC+polyA+polyG":
        reads = reads + rolled(3000, [A, C]) + repeat_reads(500, [A]) + repeat_reads(200, [G]) + repeat_reads(90, [T])
    else:
        reads = reads + rolled(3000, UNITS[kind])
    plan = go(engine, "count", reads, k, m, OPTS)
    assert beside(plan) == periodic_windows(reads, k)


@pytest.mark.parametrize("k", [19, 20, 21])
@pytest.mark.parametrize("case", ["one window", "two keys", "twice", "one window, tags"])
def test_count_exact_small_counts(engine, case, k):
    m, opts = 2, dict(OPTS)
    rng = np.random.default_rng(4)
    r = stretch_read(rng, [A, C], k + 2 if case == "two keys" else k + 1, 30)
    reads = fixed_library("pe100", 13) + [r] + ([r.copy()] if case == "twice" else [])
    if case == "one window, tags":
        opts["s1_skm_tags"] = 1
    plan = go(engine, "count", reads, k, m, opts)
    assert beside(plan) == periodic_windows(reads, k)


@pytest.mark.parametrize("case", ["first base", "last base", "different bases in front"])
def test_count_a_solid_key_without_an_edge_takes_the_prefix_plan(engine, case):
    """'$' is not tallied: a window at a read's first (last) base, seen twice, is solid without an in- (out-) edge; so is a stretch of k + 2
    bases in two reads with different bases in front.  Such a key raises the flag and the prefix plan does the job, as for homopolymers"""
    k = 21
    rng = np.random.default_rng(5)
    if case == "different bases in front":
        r = stretch_read(rng, [A, C], k + 2, 30)
        r2 = r.copy()
        r2[29] = (int(r[29]) + 1) % 4
        if r2[29] == r[30 + 1]:  # (the base the repeat would have there: keep the stretch at k + 2 bases)
            r2[29] = (int(r2[29]) + 1) % 4
        extra = [r, r2]
    else:
        r = stretch_read(rng, [A, C], k + 1, 0 if case == "first base" else 100 - (k + 1))
        extra = [r, r.copy()]
    reads = fixed_library("pe100", 23) + extra
    go(engine, "count", reads, k, 2, OPTS, want_plan="count: stream", want_kernels=COUNT_KERNELS + ("count_groups",), absent=())


# ---- 10: seeded random ----
@pytest.mark.parametrize("i", range(40))
def test_seeded_random_libraries(engine, i):
    """0 .. 4 planted units of period 1 .. 6, whole reads or stretches inside random reads, 1 .. 2000 of each; about answers, not routes"""
    rng = np.random.default_rng([20261019, i])
    what = "count" if rng.random() < 0.5 else "stage 1"
    k, m = int(rng.integers(19, 22 if what == "count" else 23)), int(rng.integers(1, 3))
    reads = fixed_library("pe100", 100 + i)
    for _ in range(int(rng.integers(0, 5))):
        unit = rng.integers(0, 4, size=int(rng.integers(1, 7)), dtype=np.uint8)
        n = int(rng.choice([1, 2, 3, 17, 300, 2000]))
        if rng.random() < 0.5:
            new = rolled(n, unit)
            reads = reads + (revcomp(new[: n // 3]) + new[n // 3:] if rng.random() < 0.5 else new)
        else:
            reads = reads + [stretch_read(rng, unit, int(rng.integers(k - 2, 70)), int(rng.integers(0, 31))) for _ in range(min(n, 300))]
    opts = dict(OPTS, s1_skm_max_bin=1 << 30)
    if what == "count":
        plan = go(engine, what, reads, k, m, opts, want_plan="count: ", want_kernels=("count_skm_make", "count_skm_rep"), absent=())
    else:
        plan = go(engine, what, reads, k, m, opts)
    if plan.startswith(("super-k-mers", "count: super-k-mers")):
        assert beside(plan) == periodic_windows(reads, k)


# ---- 11: the command line ----
@pytest.mark.parametrize("prog", ["read2sdbg", "count"])
def test_cli_reproduces_the_golden_digests(prog, tmp_path, monkeypatch):
    ent = [e for e in gu.cases() if e["case"]["prog"] == prog and e["case"]["lib"] == "r3" and e["case"]["k"] == 21 and e["case"]["m"] == 2 and
           not e["case"].get("mercy")][0]
    for name, v in dict(MHX_S1_SKM="2", MHX_S1_SKM_REP="1", MHX_NUM_GPUS="1").items():
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
    assert logs and "windows of period <= 4 beside the records" in logs[-1], logs[-1][-2000:]


# ---- 12: several ranks ----
def test_several_ranks_give_the_path_up_together_with_the_option_on():
    """the option is for one GPU: on two ranks the (AC)n reads fill a bin as before, the ranks take the pre-sorted exchange of the prefix
    plan together, and the answer is the oracle's"""
    from test_gpu_comm import run_ranks, sdbg_of, check_sdbg as check_ranks
    world, k = 2, 21
    lib_ = case_library("route", 11)[0]
    reads = [lib_[r::world] for r in range(world)]

    def load_r(r, e):
        pkg = ob.Package(reads[r], reverse=True)
        e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())

    def body(r, e, cm):
        from megahit_amd import lib
        cm.setup(0, k, 2)
        cm.read2sdbg(k, 2)
        return sdbg_of(e) + (e.fetch(lib.BUF_MUL_HIST, np.int64), e.last_s1_plan())

    outs = run_ranks(world, load_r, body, dict(OPTS))
    pkg = ob.Package(reads[0] + reads[1], reverse=True)
    s1 = ob.s1(pkg, k, 2)
    for o in outs:
        assert o[5].startswith("stream") and "pre-sorted exchange" in o[5] and "super-k-mer records given up" in o[5], o[5]
    assert np.array_equal(sum(o[4] for o in outs), s1["hist"])
    check_ranks(outs, ob.s2(pkg, k, 2, s1["is_solid"]))
