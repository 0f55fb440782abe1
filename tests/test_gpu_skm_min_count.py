"""GPU: min count 3 and 4 on super-k-mer records (s1_skm_max_m; megahit_amd/csrc/s1_skm.hip, the LOOK form of k_s1_skm and the four-level
form of k_count_skm).  Stage 1: a key of count 1 < c < m has c windows to mark and its slot keeps the position of one — a round that holds
such a key expands its records a second time and every window whose key is below m marks itself.  Count: the in / out tallies per
neighbouring base climb to four.  Against the oracle (what run / run_count of test_gpu_skm compare: is_solid, histogram, item count, the
SdBG of stage 2; edges, buckets, first_0_out / last_0_in), on libraries whose histogram bins 2 and 3 hold thousands of keys, under the
option sets that make rounds overflow and split, on constructed reads (a read twice, thrice, with its reverse complement, two records of
one read, two windows of one record, homopolymer keys of count 3 and of count 2 — the give-up), what the knob leaves alone, the command
line, and ten seconds of random libraries."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import oracle_binding as ob
from megahit_amd import lib, synth
from test_gpu_count import load, make_reads
from test_gpu_round3_knobs import fixed_library
from test_gpu_skm import repeat_reads, run, run_count
from test_gpu_skm_rep import stretch_read

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTS = dict(s1_skm=2, s1_skm_max_bin=1 << 30, s1_skm_max_m=4)
A, C, G, T = 0, 1, 2, 3
GIVEN_UP = "super-k-mer records given up: a key beside the records has 2 windows, below the min count"


def go(engine, what, reads, k, m, opts, **kw):
    """one run with s1_skm_max_m (and s1_skm_rep) put back afterwards — the RESET of test_gpu_skm does not know them; -> the plan line of
    stage 1 / of count, taken when that call returns"""
    name = "count" if what == "count" else "read2sdbg_s1"
    call, plans = getattr(engine, name), []

    def keeping_the_plan(*a, **kwa):
        r = call(*a, **kwa)
        plans.append(engine.last_s1_plan())
        return r

    setattr(engine, name, keeping_the_plan)
    try:
        if what == "count":
            run_count(engine, reads, k, m, opts, **kw)
        else:
            run(engine, reads, k, m, opts, **kw)
        return plans[-1]
    finally:
        delattr(engine, name)
        engine.set_option("s1_skm_max_m", 2)
        engine.set_option("s1_skm_rep", 0)


OPTION_SETS = [dict(), dict(s1_stream_fill=40), dict(s1_stream_fill=3), dict(s1_stream_probes=2), dict(s1_skm_tags=1), dict(s1_skm_bin_bits=18), dict(s1_skm_passes=3),
               dict(s1_skm_deal=0)]
IDS = dict(ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "default")


# ---- the libraries: histogram bins 2 and 3 (keys of count 2 / 3) as the oracle counts them, so the second look and the upper levels have work
@pytest.mark.parametrize("opts", OPTION_SETS, **IDS)
@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 3),        # 6260 / 261
                                      ("repeats100", 21, 3),   # 3659 / 607
                                      ("short30", 21, 3),      # 5 / 6
                                      ("tiny60", 21, 3),       # 0 / 0: every key non-solid
                                      ("pe100", 19, 4),        # 5320 / 335
                                      ("repeats100", 22, 4),   # 3501 / 615
                                      ("pe100", 20, 3)])       # 6130 / 261
def test_stage1_at_min_count_3_and_4(engine, kind, k, m, opts):
    """s1_stream_fill = 40 and 3: rounds that overflow are redone in halves by the second hash — the look takes the round's own windows only;
    s1_skm_deal = 0 is not consulted at min count 3 and 4 (nor is the 1 that test_gpu_skm leaves behind): same kernels, same answer"""
    go(engine, "stage 1", fixed_library(kind, seed=k * 7 + m), k, m, dict(OPTS, **opts))


@pytest.mark.parametrize("opts", OPTION_SETS, **IDS)
@pytest.mark.parametrize("kind,k,m", [("pe100", 21, 3),        # 5634 / 290
                                      ("repeats100", 21, 3),   # 3242 / 433
                                      ("short30", 21, 3),      # 4 / 16
                                      ("tiny60", 20, 3),       # 0 / 0: no edge at all
                                      ("pe100", 19, 4),        # 5846 / 331
                                      ("repeats100", 21, 4)])  # 3218 / 727
def test_count_at_min_count_3_and_4(engine, kind, k, m, opts):
    go(engine, "count", fixed_library(kind, seed=k * 11 + m), k, m, dict(OPTS, **opts))


# ---- constructed reads beside fixed_library("pe100", 13) ----
def c_read(n_c, k=21):
    """a random read with exactly n_c bases of C from base 30 on (A in front, T behind)"""
    r = np.random.default_rng(4).integers(0, 4, size=100, dtype=np.uint8)
    r[30:30 + n_c] = C
    r[29], r[30 + n_c] = A, T
    return r


def constructed(case, k=21):
    rng = np.random.default_rng(41)
    r = rng.integers(0, 4, size=100, dtype=np.uint8)
    if case == "a read twice":  # + 79 keys of count 2: all its windows are marked, from records of two reads
        return [r, r.copy()], 3
    if case == "a read three times":  # + 79 of count 3, non-solid at 4
        return [r, r.copy(), r.copy()], 4
    if case == "a read and its reverse complement":  # + 79 of count 2, occurrences on both strands
        return [r, (3 - r[::-1]).astype(np.uint8)], 3
    if case == "X.Y.X":  # + 9 keys of count 2: two records of one read
        x, y = rng.integers(0, 4, size=30, dtype=np.uint8), rng.integers(0, 4, size=40, dtype=np.uint8)
        return [np.concatenate([x, y, x])], 3
    if case == "period 5":  # + 1 key of count 2: its two windows are five apart and can share one record; beyond s1_skm_rep
        return [stretch_read(rng, [A, C, G, T, T], k + 6, 30)], 3
    raise ValueError(case)


@pytest.mark.parametrize("what", ["stage 1", "count"])
@pytest.mark.parametrize("case", ["a read twice", "a read three times", "a read and its reverse complement", "X.Y.X", "period 5"])
def test_constructed_reads(engine, case, what):
    extra, m = constructed(case)
    go(engine, what, fixed_library("pe100", 13) + extra, 21, m, OPTS)


def test_a_homopolymer_key_of_count_3_is_solid(engine):
    """exactly k + 3 bases of C inside a random read: three windows of the one key counted beside the records — solid at 3, the path holds"""
    go(engine, "stage 1", fixed_library("pe100", 13) + [c_read(21 + 3)], 21, 3, OPTS)


def test_a_homopolymer_key_of_count_2_gives_the_job_up(engine):
    """exactly k + 2 bases of C: the key has two windows and the tally beside the records keeps the position of one.  The job goes to the
    prefix plan, whose plan line says why; a caller that left the plan to the path (s1_skm = 3) gets the error; count's tallies are exact
    and it stays on the path"""
    reads = fixed_library("pe100", 13) + [c_read(21 + 2)]
    go(engine, "stage 1", reads, 21, 3, OPTS, want_plan="stream", want_kernels=("s1_skm_make", "s1_groups"), absent=("s1_skm_groups",), why=GIVEN_UP)
    load(engine, ob.Package(reads, reverse=True))
    try:
        for n, v in dict(OPTS, s1_skm=3).items():
            engine.set_option(n, v)
        with pytest.raises(lib.MhxError, match="a key beside the records has 2 windows, below the min count"):
            engine.read2sdbg_s1(21, 3)
    finally:
        for n, v in dict(s1_skm=1, s1_skm_max_bin=65536, s1_skm_max_m=2).items():
            engine.set_option(n, v)
    go(engine, "count", reads, 21, 3, OPTS)


@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_reads_of_several_lengths(engine, what):
    """3123 keys of count 2"""
    go(engine, what, make_reads("var", 17), 21, 3, dict(OPTS, s1_var_min_fill=5, **(dict(s1_skm_cap_pct=300) if what == "count" else {})))


@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_with_the_windows_of_period_4_beside_the_records(engine, what):
    """s1_skm_rep: the (AC)n keys of 3000 reads are far above the min count and the path holds"""
    kernels = ("count_skm_make", "count_skm_groups", "count_skm_rep") if what == "count" else ("s1_skm_make", "s1_skm_groups", "s1_skm_rep")
    plan = go(engine, what, fixed_library("pe100", 13) + repeat_reads(3000, [A, C]), 21, 3, dict(OPTS, s1_skm_rep=1), want_kernels=kernels)
    assert "windows of period <= 4 beside the records" in plan, plan


# ---- what the feature leaves alone ----
@pytest.mark.parametrize("what", ["stage 1", "count"])
@pytest.mark.parametrize("how", ["knob unset, m 3", "knob 4, m 5"])
def test_beyond_the_knob_the_prefix_plan_serves(engine, what, how):
    opts, m = (dict(s1_skm=2), 3) if how == "knob unset, m 3" else (dict(s1_skm=2, s1_skm_max_m=4), 5)
    reads = fixed_library("pe100", 13)
    load(engine, ob.Package(reads, reverse=True))
    try:
        for n, v in opts.items():
            engine.set_option(n, v)
        assert not engine.s1_self_planned(21, m) and not engine.count_self_planned(21, m)
        if how == "knob 4, m 5":
            assert engine.s1_self_planned(21, 3) and engine.s1_self_planned(21, 4) and engine.count_self_planned(21, 3) and engine.count_self_planned(21, 4)
            assert not engine.s1_self_planned(21, 3, want_mercy=True) and not engine.count_self_planned(22, 3)
    finally:
        engine.set_option("s1_skm", 1)
        engine.set_option("s1_skm_max_m", 2)
    if what == "count":
        plan = go(engine, what, reads, 21, m, opts, want_plan="count: ", want_kernels=("count_groups",), absent=("count_skm_make", "count_skm_groups"))
        assert not plan.startswith("count: super-k-mers"), plan
    else:
        plan = go(engine, what, reads, 21, m, opts, want_plan="", want_kernels=(), absent=("s1_skm_make", "s1_skm_groups"))
        assert not plan.startswith("super-k-mers"), plan


@pytest.mark.parametrize("what", ["stage 1", "count"])
def test_the_knob_at_min_count_2_changes_nothing(engine, what):
    """plan, kernel names and results as without it"""
    go(engine, what, fixed_library("pe100", 13), 21, 2, OPTS)


def test_values_outside_2_to_4_mean_the_nearest(engine):
    reads = fixed_library("pe100", 13)
    load(engine, ob.Package(reads, reverse=True))
    try:
        engine.set_option("s1_skm", 2)
        for knob, served in ((0, 2), (1, 2), (3, 3), (9, 4)):
            engine.set_option("s1_skm_max_m", knob)
            assert [bool(engine.s1_self_planned(21, m)) for m in (2, 3, 4, 5)] == [m <= served for m in (2, 3, 4, 5)], knob
    finally:
        engine.set_option("s1_skm", 1)
        engine.set_option("s1_skm_max_m", 2)


# ---- the command line ----
@pytest.mark.parametrize("prog", ["read2sdbg", "count"])
def test_cli_writes_the_same_files_on_either_route(prog, tmp_path, monkeypatch):
    """mhx_core -k 21 -m 3 with and without MHX_S1_SKM_MAX_M=4: byte-identical output files, the group-by on super-k-mer records in the
    profile of the run with the knob only"""
    reads = synth.gen_pe_reads(3000, 8000, read_len=100, frag=250, err=0.01, seed=13)
    synth.write_read_lib(str(tmp_path / "reads"), [reads])
    for name, v in dict(MHX_S1_SKM="2", MHX_NUM_GPUS="1", MHX_PROFILE="1").items():
        monkeypatch.setenv(name, v)
    kernel = "s1_skm_groups" if prog == "read2sdbg" else "count_skm_groups"
    logs = {}
    for knob in ("2", "4"):
        out = tmp_path / ("out" + knob)
        out.mkdir()
        monkeypatch.setenv("MHX_S1_SKM_MAX_M", knob)
        p = subprocess.run([gu.MHX_CORE, prog, "-k", "21", "-m", "3", "--host_mem", "2e9", "--num_cpu_threads", "3", "--read_lib_file", str(tmp_path / "reads"),
                            "--output_prefix", str(out / "o")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[knob] = p.stderr
    names = sorted(os.listdir(tmp_path / "out2"))
    assert names and names == sorted(os.listdir(tmp_path / "out4"))
    for n in names:
        assert filecmp.cmp(tmp_path / "out2" / n, tmp_path / "out4" / n, shallow=False), n
    assert kernel in logs["4"], logs["4"][-2000:]
    assert kernel not in logs["2"], logs["2"][-2000:]


# ---- random libraries ----
def test_ten_seconds_of_random_libraries_at_min_count_3_and_4():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_skm.py"), "--min-count", "10", "91000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "all equal to the oracle" in p.stdout, p.stdout[-1500:]
