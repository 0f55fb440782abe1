"""GPU: the memory plan is held to its budget.  mhx_core cuts a stage into passes over lv1 bucket ranges from one figure per stage, the
device bytes a pass holds per kept item (mhx_stage_pass_bytes, mhx_stage_once_bytes, plan_ranges in host/mhx_core.cpp, plan_dist_passes
in comm.hip).  Here the figure is compared with what the stages allocate, counted where every device allocation passes (mhx_alloc_peak):

(a) through an Engine, the growth of the peak with the kept items against the growth of the model;
(b) through mhx_core with a faked small device (MHX_FREE_BYTES), `peak - held when planned <= budget` for every stage line of every run,
    with the planned pass counts and the outputs of the unplanned run;
(c) the same for two ranks.

No allocation is made to fail: every run allocates megabytes on a device with hundreds of gigabytes and is judged by the counter.

The libraries: 200 000 reads of 100 bases (20 M bases) and 236 000 reads of 70 to 100 bases (20 M bases) of a random genome of 2 M
bases, so no lv1 bucket holds more than a few thousand items."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
from megahit_amd import canon, lib, synth

pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")

GENOME = 2000000
READ_LEN = 100
NB = lib.NUM_BUCKETS


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """{"fixed" / "var": (prefix of the read library files, reads, bases)} and "genome": the genome (uint8)"""
    d = str(tmp_path_factory.mktemp("memplan"))
    genome = np.random.default_rng(41).integers(0, 4, size=GENOME, dtype=np.uint8)
    out = {"genome": genome, "dir": d}
    fixed = synth.gen_pe_reads(100000, GENOME, read_len=READ_LEN, frag=250, err=0.005, seed=42, genome=genome)
    out["fixed"] = (os.path.join(d, "fixed"),) + synth.write_read_lib(os.path.join(d, "fixed"), [fixed])
    var = synth.gen_pe_reads(118000, GENOME, read_len=READ_LEN, frag=250, err=0.005, seed=43, genome=genome)
    lens = np.random.default_rng(44).integers(70, READ_LEN + 1, size=var.shape[0]).astype(np.uint32)
    out["var"] = (os.path.join(d, "var"),) + synth.write_var_read_lib(os.path.join(d, "var"), [(var, lens)])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the per-item figure, through the Engine
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine_with_reads(libs, which):
    prefix, n_reads, _ = libs[which]
    e = lib.Engine(0)
    e.load_bin_records(np.fromfile(prefix + ".bin", dtype=np.uint32), n_reads)
    return e


def _contig_windows(genome, length, step):
    """overlapping windows of the genome as contigs -> (packed words, start positions, multiplicities)"""
    starts = np.arange(0, genome.size - length, step)
    bases = genome[starts[:, None] + np.arange(length)[None, :]]
    return synth.pack_reads_concat(bases), (np.arange(starts.size + 1, dtype=np.uint64) * np.uint64(length)), np.full(starts.size, 3, dtype=np.uint16)


def _engine_with_edges_and_contigs(libs, k):
    """what seq2sdbg reads: the solid edges a count of the fixed-length library wrote (k = 29; at k = 99 a read holds one (k+1)-mer and
    next to none is solid) and contigs, here windows of the genome of 2000 bases every 1000"""
    e = lib.Engine(0)
    words, start, mult = _contig_windows(libs["genome"], 2000, 1000)
    if k + 1 >= READ_LEN:
        e.load_sequences(words, mult.size, 0, start)
        e.load_multiplicity(mult)
        return e
    prefix, n_reads, _ = libs["fixed"]
    e.load_bin_records(np.fromfile(prefix + ".bin", dtype=np.uint32), n_reads)
    r = e.count(k, 2)
    edges = e.fetch(lib.BUF_EDGES, np.uint32).reshape(-1, r.words_per_edge)
    j = np.arange(k + 1)
    bases = ((edges[:, j >> 4] >> (30 - 2 * (j & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    e.close()
    e = lib.Engine(0)
    e.load_sequences(synth.pack_reads_concat(bases), bases.shape[0], k + 1, None)
    e.load_multiplicity((edges[:, -1] & 0xFFFF).astype(np.uint16))
    e.append_sequences(words, mult.size, 0, start, mult)
    return e


# (id, library, stage for the model and the histogram, k, m, what runs)
ENGINE_CASES = [
    ("s1-k21-fixed", "fixed", lib.STAGE_S1, 21, 2, "s1"),
    ("s1-k21-var", "var", lib.STAGE_S1, 21, 2, "s1"),
    ("s1-k31-fixed", "fixed", lib.STAGE_S1, 31, 2, "s1"),
    ("s1-mercy-k21", "fixed", lib.STAGE_S1_MERCY, 21, 2, "s1_mercy"),
    ("count-k21", "fixed", lib.STAGE_COUNT, 21, 2, "count"),
    ("count-k31", "fixed", lib.STAGE_COUNT, 31, 2, "count"),
    ("s2-k21-m2-aggregated", "fixed", lib.STAGE_S2, 21, 2, "s2"),
    ("s2-k27-m2", "fixed", lib.STAGE_S2, 27, 2, "s2"),
    ("s2-k27-m1", "fixed", lib.STAGE_S2, 27, 1, "s2"),
    ("seq2sdbg-k29", "edges", lib.STAGE_SEQ2SDBG, 29, 0, "seq2sdbg"),
    ("seq2sdbg-k99", "edges", lib.STAGE_SEQ2SDBG, 99, 0, "seq2sdbg"),
]


def _measure(libs, which, stage, k, m, what, n_target):
    """One filtered pass over the lv1 buckets [0, hi) that hold about n_target items, on an Engine of its own (grow-only buffers of an
    earlier pass would hide this one's allocations): -> (kept items, peak - held before, the model's bytes)"""
    e = _engine_with_edges_and_contigs(libs, k) if which == "edges" else _engine_with_reads(libs, which)
    try:
        if what == "s2" and m > 1:
            e.read2sdbg_s1(k, m)  # the bitmap (and, k <= 22, the aggregated items) stage 2 starts from: held before, not part of the pass
        cum = np.cumsum(e.bucket_histogram(stage, k, m))
        if n_target is None:  # about a quarter of all items, 2 M at the most
            n_target = min(2000000, int(cum[-1]) // 4 - int(cum[-1]) // 64)
        hi = min(NB, int(np.searchsorted(cum, n_target)) + 1)
        items = int(cum[hi - 1])
        keep = np.zeros(NB, dtype=np.uint8)
        keep[:hi] = 1
        e.trim()
        held, _ = e.alloc_peak(reset=True)
        e.set_bucket_filter(keep, expected_items=items)
        model = e.stage_pass_bytes(stage, k, m, items)
        if what == "s1":
            e.read2sdbg_s1(k, m)
        elif what == "s1_mercy":
            e.read2sdbg_s1(k, m, want_mercy=2)
        elif what == "count":
            e.count(k, m)
        elif what == "s2":
            e.read2sdbg_s2(k, m)
        else:
            e.seq2sdbg(k)
        _, peak = e.alloc_peak()
        e.set_bucket_filter(None)
        return items, n_target, peak - held, model
    finally:
        e.close()


@pytest.mark.parametrize("case", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_peak_grows_no_faster_than_the_model(libs, case):
    """Three passes over n, 2n and 4n kept items (n = 2 M, or a sixteenth short of a quarter of the stage's items where it has fewer
    than 8 M): from each to the next the peak may grow by no more than the model does,

        peak(larger) - peak(smaller) <= (model(larger) - model(smaller)) * (1 + 1/16) + 64 KiB.

    1/16 is the headroom DevBuf::reserve adds to every allocation (bytes + bytes / 16 + 256); 64 KiB covers its 256 bytes on some 250
    buffers.  The differences cancel the fixed state (bitmaps, per-read tables, 64 Ki-entry tables, the filter's tables): no measured
    constant enters.  model / measured of the growth is printed, not asserted (memory plan)."""
    _, which, stage, k, m, what = case
    runs, n = [], None
    for mul in (1, 2, 4):
        items, n0, got, model = _measure(libs, which, stage, k, m, what, None if n is None else n * mul)
        n = n0 if n is None else n
        runs.append((items, got, model))
    for (i0, g0, m0), (i1, g1, m1) in zip(runs, runs[1:]):
        print("memory-plan figure %s: items %d -> %d, peak grows %d bytes (%.2f per item), model %d (%.2f per item), model / measured %.3f"
              % (case[0], i0, i1, g1 - g0, (g1 - g0) / (i1 - i0), m1 - m0, (m1 - m0) / (i1 - i0), (m1 - m0) / max(1, g1 - g0)))
    for (i0, g0, m0), (i1, g1, m1) in zip(runs, runs[1:]):
        assert i1 > i0 and m1 > m0
        assert g1 - g0 <= (m1 - m0) * (1 + 1 / 16) + 65536, (case[0], i0, i1, g1 - g0, m1 - m0)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the budget, through mhx_core
# ---------------------------------------------------------------------------------------------------------------------------------
STAGE_LINE = re.compile(r"Device memory of ([^:]+): (\d+) bytes held when planned, peak (\d+) bytes, budget (\d+)")
PLAN_LINE = re.compile(r"Memory plan: (\d+) passes over lv1 bucket ranges")


def _stages(stderr):
    """-> [(stage, held when planned, peak, budget, passes)] in the order of the run; a stage's `Memory plan:` line, if any, stands
    between the previous stage's line and its own"""
    out, passes = [], 1
    for line in stderr.splitlines():
        mp = PLAN_LINE.search(line)
        if mp:
            passes = int(mp.group(1))
        ms = STAGE_LINE.search(line)
        if ms:
            out.append((ms.group(1), int(ms.group(2)), int(ms.group(3)), int(ms.group(4)), passes))
            passes = 1
    return out


def _core(binary, args, out, env=None, threads="3"):
    p = subprocess.run([binary] + args + ["--output_prefix", out, "--host_mem", "2e9", "--num_cpu_threads", threads], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert p.returncode == 0, "exit %d\n%s" % (p.returncode, p.stderr[-2000:])
    return p.stderr


def _digests(prog, out):
    if prog == "count":
        return {"edges": canon.digest_edges(out), "cand": canon.digest_file(out + ".cand"), "counting": canon.digest_file(out + ".counting")}
    d = {"sdbg": canon.digest_sdbg(out)}
    if os.path.exists(out + ".counting"):
        d["counting"] = canon.digest_file(out + ".counting")
    return d


# Where the factors c of MHX_FREE_BYTES = c * B come from (B: the bases of the stage's input; everything per base of the input).
# plan_ranges has avail = 0.8 * c - fixed - 17/16 * (the library's figure for no items + two staging batches of c / 32 each)
#   = 0.7336 * c - fixed', and per_item' = 17/16 * per_item (the allocator's headroom); one pass if per_item' * bound <= avail,
#   else passes of at most avail / per_item' items.  The tables of the giant buckets, 32 MiB, are 1.68 per base of these 20 M.
#   stage 1: the generating first sort pass, for reads of one length and of several: per_item 24.5 (two 12-byte record buffers + status
#     words) + 0.25 (giant buckets' partial sums) + 8 at k <= 22 (the kept buckets' aggregated stage-2 items at their bound): per_item'
#     34.8 at k = 21, 26.3 at k = 27; bound 1.04 (a base + 4 per read of 100; 1.047 for reads of 85 on average); fixed' = 1 + 1/8
#     (+ 1 at k <= 22) + 17/16 * (0.347 status words over all item slots + 1.68): 4.28 at k = 21, 3.28 at k = 27; the library has
#     (100 - k + 3) / 100 items per base: 0.82 at k = 21, 0.76 at k = 27; 0.79 at k = 21 for the reads of several lengths
#   stage 1 with mercy, k = 31: per_item' 17/16 * (3 * 24 + 1) = 77.6, bound 1.04, fixed' 1.125; 0.72 items
#   count, k = 21: per_item 24.5 + 0.25 + 12 (the kept buckets' solid edges at their bound: one of 8 bytes per 2 items, three buffers):
#     per_item' 39.05; bound 1; fixed' = 0.12 (12 per read) + 17/16 * (0.333 + 2 * 1.68) = 4.04; 0.79 items
#   count, k = 31 (two-word keys take the 16-byte items): per_item' 17/16 * (3 * 16 + 1) = 52.06, fixed' 0.12; 0.69 items
#   stage 2, k = 27: per_item' 17/16 * (3 * 8 + 1) = 26.56 in passes, bound 2.2; once, from a count of the (k+1)-mers: 17/16 * 13 * 2.2
#     = 30.4; the library has two items per solid (k+1)-mer occurrence and the dummies: 1.3 (min count 2), 1.46 (min count 1)
#   seq2sdbg, k = 29, edges of 30 bases: per_item' 52.06, bound 2 + 4 / 30 = 2.133; 6 items per edge (seq_to_sdbg.cpp:530-577:
#     both strands of the edge and of its two ends): 0.2
# (c_passes: the stage under test in 3 to 6 passes; c_once: a few per cent over (per_item' * bound + fixed') / 0.7336)
#   (id, program, library, k, m, mercy, stage under test, c_passes, c_once)
CORE_CASES = [
    # (0.7336 * 15.4 - 4.28) / 34.8 = 0.202 items per pass of 0.82: 5;  (34.8 * 1.04 + 4.28) / 0.7336 = 55.2
    ("read2sdbg-k21-m2", "read2sdbg", "fixed", 21, 2, False, "stage 1", 15.4, 57),
    # (0.7336 * 15 - 4.28) / 34.8 = 0.193 of 0.79: 5;  (34.8 * 1.047 + 4.28) / 0.7336 = 55.5
    ("read2sdbg-k21-m2-var", "read2sdbg", "var", 21, 2, False, "stage 1", 15, 57),
    # stage 2: 0.7336 * 12.7 / 26.56 = 0.35 of 1.3: 4;  once 30.4 / 0.7336 = 41.4, stage 1 (26.3 * 1.04 + 3.28) / 0.7336 = 41.8
    ("read2sdbg-k27-m2", "read2sdbg", "fixed", 27, 2, False, "stage 2", 12.7, 43),
    # stage 2 alone: 0.7336 * 14.5 / 26.56 = 0.40 of 1.46 (every occurrence is an item): 4;  30.4 / 0.7336 = 41.4
    ("read2sdbg-k27-m1", "read2sdbg", "fixed", 27, 1, False, "stage 2", 14.5, 43),
    # (0.7336 * 20.6 - 1.125) / 77.6 = 0.18 of 0.72: 4 or 5;  (77.6 * 1.04 + 1.125) / 0.7336 = 111.5
    ("read2sdbg-k31-m2-mercy", "read2sdbg", "fixed", 31, 2, True, "stage 1 (mercy)", 20.6, 115),
    # (0.7336 * 15.7 - 4.04) / 39.05 = 0.19 of 0.79: 5;  (39.05 + 4.04) / 0.7336 = 58.7
    ("count-k21-m2", "count", "fixed", 21, 2, False, "count", 15.7, 61),
    # (0.7336 * 12.4 - 0.12) / 52.06 = 0.172 of 0.69: 4 or 5;  (52.06 + 0.12) / 0.7336 = 71.1
    ("count-k31-m2", "count", "fixed", 31, 2, False, "count", 12.4, 73.5),
    # 0.7336 * 3.55 / 52.06 = 0.05 of 0.2: 4;  52.06 * 2.133 / 0.7336 = 151.4
    ("seq2sdbg-k29", "seq2sdbg", "fixed", 29, 2, False, "seq2sdbg", 3.55, 156),
]
REF_CASES = ("read2sdbg-k21-m2", "count-k21-m2", "seq2sdbg-k29")

_unplanned = {}


def _args(case, libs, workdir):
    """-> (arguments of the sub-program, bases of its input)"""
    cid, prog, which, k, m, mercy, _, _, _ = case
    prefix, _, bases = libs[which]
    if prog != "seq2sdbg":
        return [prog, "-k", str(k), "-m", str(m), "--read_lib_file", prefix] + (["--need_mercy"] if mercy else []), bases
    cnt = os.path.join(libs["dir"], "cnt_k%d" % k)  # the edges a count of the same library wrote, made once
    if not os.path.exists(cnt + ".edges.info"):
        _core(gu.MHX_CORE, ["count", "-k", str(k), "-m", str(m), "--read_lib_file", prefix], cnt)
    n_edges = int(canon.canonical_edges(cnt)[1].shape[0])
    return ["seq2sdbg", "-k", str(k), "--kmer_from", "0", "--input_prefix", cnt], n_edges * (k + 1)


def _unplanned_run(case, libs):
    """the run without a plan, once per case: -> (digests, its stage lines)"""
    if case[0] not in _unplanned:
        args, _ = _args(case, libs, libs["dir"])
        out = os.path.join(libs["dir"], "unplanned_" + case[0])
        err = _core(gu.MHX_CORE, args, out)
        _unplanned[case[0]] = (_digests(case[1], out), _stages(err))
    return _unplanned[case[0]]


def _check_budget(stages, factor=1):
    assert stages, "no `Device memory of <stage>` line"
    for stage, held, peak, budget, passes in stages:
        print("memory-plan budget: %s, %d passes: peak - held = %d, budget %d (%.3f of it)" % (stage, passes, peak - held, budget, (peak - held) / budget))
    for stage, held, peak, budget, passes in stages:
        assert peak - held <= factor * budget, (stage, passes, peak - held, budget)


@pytest.mark.parametrize("fit", ["passes", "once"])
@pytest.mark.parametrize("case", CORE_CASES, ids=[c[0] for c in CORE_CASES])
def test_core_stays_inside_its_budget(libs, case, fit, tmp_path):
    """`mhx_core` on a device faked small: every stage of the run holds, over what was held when its plan was made, at most the free
    bytes it planned with — a process that exceeds them on a device with that much free memory gets a hipMalloc failure.  The plan aims
    at 0.8 of them, which leaves a quarter; nothing else is allowed for.  "passes": the stage under test runs in 3 to 6 passes;
    "once": the budget is a few per cent above what one pass needs by the model, and one pass it is.  The outputs are those of the
    run without a plan, and no lv1 bucket was tried alone above the budget."""
    cid, prog, which, k, m, mercy, under_test, c_passes, c_once = case
    want, _ = _unplanned_run(case, libs)
    args, bases = _args(case, libs, str(tmp_path))
    out = str(tmp_path / "out")
    err = _core(gu.MHX_CORE, args, out, env={"MHX_FREE_BYTES": str(int((c_passes if fit == "passes" else c_once) * bases))})
    stages = _stages(err)
    print("\n".join(line for line in err.splitlines() if "Memory plan" in line or "Device memory of" in line))
    assert "alone holds" not in err, err[-2000:]
    mine = [s for s in stages if s[0] == under_test]
    assert len(mine) == 1, stages
    if fit == "passes":
        assert 3 <= mine[0][4] <= 6, stages
    else:
        assert mine[0][4] == 1, stages
    _check_budget(stages)
    assert _digests(prog, out) == want


def test_unplanned_runs_report_their_stages(libs):
    """without MHX_FREE_BYTES the lines are there too, with the device's free bytes as the budget"""
    for case in (CORE_CASES[0], CORE_CASES[5]):
        _, stages = _unplanned_run(case, libs)
        assert [s[0] for s in stages] == (["stage 1", "stage 2"] if case[1] == "read2sdbg" else ["count"]), stages
        _check_budget(stages)


@needs_ref
@pytest.mark.parametrize("case", [c for c in CORE_CASES if c[0] in REF_CASES], ids=REF_CASES)
def test_unplanned_run_equals_the_reference(libs, case, tmp_path):
    """what the planned runs are compared with is what the reference binary writes (one case per program)"""
    want, _ = _unplanned_run(case, libs)
    args, _ = _args(case, libs, str(tmp_path))
    out = str(tmp_path / "ref")
    _core(REF, args, out)
    assert _digests(case[1], out) == want


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) two ranks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_inside_their_budgets(libs, tmp_path):
    """`mhx_core --gpus 2 read2sdbg` at (21, 2), both ranks on device 0 behind the in-process transport.  A rank plans with
    4 * item_bytes + 1 = 49 bytes per item of 0.8 * MHX_FREE_BYTES = 12 per base: 0.24 items per base a pass, of the 0.41 a rank owns
    or extracts.  The counter is the process's, so the two ranks together may hold 2 * budget."""
    case = CORE_CASES[0]
    want, _ = _unplanned_run(case, libs)
    args, bases = _args(case, libs, str(tmp_path))
    out = str(tmp_path / "out")
    err = _core(gu.MHX_CORE, args, out, env={"MHX_FREE_BYTES": str(15 * bases), "MHX_NUM_GPUS": "2", "MHX_GPU_MAP": "0,0"})
    stages = _stages(err)
    print("\n".join(line for line in err.splitlines() if "Device memory of" in line))
    assert [s[0] for s in stages] == ["stage 1", "stage 2"], stages
    _check_budget(stages, factor=2)
    assert _digests("read2sdbg", out) == want
