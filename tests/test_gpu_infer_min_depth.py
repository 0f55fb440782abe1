"""GPU: the minimum depth `assemble` infers when none is given (include/mhx.h: mhx_sdbg_mul_histogram, mhx_infer_min_depth,
mhx_sdbg_infer_min_depth; csrc/sdbg_index.hip k_sdbg_mul_hist).  The histogram kernel against np.bincount over the fetched
MHX_BUF_SDBG_MUL / _INVALID (the existing, reference-checked buffers) on graphs at the kernel's edges; on the graphs of
tests/golden/infer_min_depth.json (tools/make_infer_min_depth_golden.py) the device histogram against the reference's own;
`mhx_core assemble` without a positive --min_depth, its route's opt-in variable at 2, against the COMMITTED digests, counts and
logged depth of the reference's own `assemble -t 1`, with MHX_REF_CORE pointing to a stub that fails, so a run that forwarded
instead of computing cannot pass; the resident server; a command line served before, unchanged; and, where
oracle/_ref/ref_megahit_core is built, fresh seeds against the reference run live, files byte for byte."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from megahit_amd import lib, synth

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_infer_min_depth_golden as mig  # noqa: E402
from test_gpu_unitig_prune import load_files_into, stub  # noqa: E402

mcg = mig.mcg
pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
with open(os.path.join(gu.GOLD, "infer_min_depth.json")) as f:
    GOLDEN = json.load(f)["cases"]
BY_NAME = {c["name"]: c for c in GOLDEN}
with open(os.path.join(gu.GOLD, "unitig_clean.json")) as f:
    CLEAN_GOLDEN = {c["name"]: c for c in json.load(f)["cases"]}
TILE = 16384  # items of a workgroup tile of k_sdbg_mul_hist


def read2sdbg(d, c, lib_prefix=None):
    """the case's library -> mhx_core read2sdbg -> the graph's prefix"""
    out = os.path.join(d, "g")
    subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", lib_prefix or mcg.write_library(d, c), "--output_prefix", out] + (["--need_mercy"] if c["mercy"] else []),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    return out


@pytest.fixture(scope="module")
def graph_of(tmp_path_factory):
    """case -> prefix of its graph (mhx_core read2sdbg), built once per library"""
    made = {}

    def get(c):
        key = tuple(c.get(k) for k in mig.LIBRARY)
        if key not in made:
            made[key] = read2sdbg(str(tmp_path_factory.mktemp("g")), c)
        return made[key]

    return get


def expected_histogram(engine, info):
    """np.bincount over the fetched multiplicities of the edges whose INVALID bit is clear; -> (hist, invalid bits [n])"""
    n = info.n_items
    mul = engine.fetch(lib.BUF_SDBG_MUL, np.uint16)
    inv = np.unpackbits(engine.fetch(lib.BUF_SDBG_INVALID, np.uint64).view(np.uint8), bitorder="little")[:n].astype(bool)
    assert mul.size == n
    return np.bincount(mul[~inv], minlength=65536).astype(np.uint64), inv


def check_histogram(engine, info):
    want, inv = expected_histogram(engine, info)
    hist, n_valid = engine.sdbg_mul_histogram(info)
    assert hist.dtype == np.uint64 and hist.shape == (65536,)
    n_c = C.c_uint64(0)  # the C call's own sum
    assert engine.lib.mhx_sdbg_mul_histogram(engine.h, C.byref(info), C.byref(n_c)) == 0 and n_c.value == n_valid
    # (an item counted from the padding behind n would show here: the padding bits of the last word are clear)
    assert n_valid == int(want.sum()) == int((~inv).sum())
    bad = np.nonzero(hist != want)[0]
    assert bad.size == 0, [(int(v), int(hist[v]), int(want[v])) for v in bad[:8]]
    assert np.array_equal(engine.fetch(lib.BUF_SDBG_MUL_HIST, np.uint64), want)
    return want


def graph_from_reads(engine, reads, k, m):
    """reads (uint8 [n, L]) -> stage 1 + 2 on the handle -> the index of the SdBG they leave in HBM"""
    import oracle_binding as ob
    pkg = ob.Package([r for r in reads], reverse=True)
    engine.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())
    engine.read2sdbg_s1(k, m)
    engine.read2sdbg_s2(k, m)
    return engine.sdbg_build_index(k)


def test_histogram_of_a_real_graph_before_and_after_tip_trimming(engine, graph_of):
    """the graph of case A: n is no multiple of 64 (the partial last word); after mhx_sdbg_remove_tips the histogram follows the
    new INVALID bits; it equals the reference's own histogram of the golden file before, and no longer after"""
    c = BY_NAME["A-p2"]
    k = load_files_into(engine, graph_of(c))
    info = engine.sdbg_build_index(k)
    assert info.n_items == c["n_items"] and info.n_items % 64 != 0 and info.n_items > TILE
    before = check_histogram(engine, info)
    assert [[int(v), int(before[v])] for v in np.nonzero(before)[0]] == c["hist"]
    assert engine.sdbg_remove_tips(info, 2 * k) > 0
    after = check_histogram(engine, info)
    assert after.sum() < before.sum()


def test_histogram_of_fewer_than_64_items(engine):
    reads = np.random.default_rng(5).integers(0, 4, size=(1, 30), dtype=np.uint8)
    info = graph_from_reads(engine, reads, 21, 1)
    assert 0 < info.n_items < 64
    want = check_histogram(engine, info)
    assert want.sum() > 0


def graph_from_library(engine, d, reads, k, m):
    """the same through a library file and mhx_core read2sdbg (many reads: the oracle's package takes them one by one)"""
    synth.write_read_lib(os.path.join(d, "reads"), [reads])
    load_files_into(engine, read2sdbg(d, dict(k=k, m=m, mercy=False), os.path.join(d, "reads")))
    return engine.sdbg_build_index(k)


def test_histogram_with_multiplicities_from_the_large_table(engine, tmp_path):
    """300 copies of one read: every edge has multiplicity 300, above the 254 a record's own byte holds"""
    reads = np.repeat(np.random.default_rng(6).integers(0, 4, size=(1, 40), dtype=np.uint8), 300, axis=0)
    info = graph_from_library(engine, str(tmp_path), reads, 21, 2)
    assert info.n_large > 0
    want = check_histogram(engine, info)
    assert want[300] > 0 and want[:255].sum() == 0


def test_histogram_at_the_saturated_multiplicity(engine, tmp_path):
    """70 000 copies: the multiplicity saturates at 65535, far above the values that have an LDS bin"""
    reads = np.repeat(np.random.default_rng(7).integers(0, 4, size=(1, 40), dtype=np.uint8), 70000, axis=0)
    info = graph_from_library(engine, str(tmp_path), reads, 21, 2)
    want = check_histogram(engine, info)
    assert want[65535] > 0 and want[:65535].sum() == 0


def test_histogram_of_a_library_with_more_than_one_workgroup_per_cu(engine, tmp_path):
    """60 000 pairs over 300 kb at m = 1: every read error leaves its own edges, some 5 M items in all — more tiles than the 256
    compute units of an MI355X, so compute units run several workgroups at once"""
    d = str(tmp_path)
    c = dict(mcg.B, G=300000, pairs=60000, err=0.01, seed=77)
    reads = synth.gen_pe_reads(c["pairs"], c["G"], read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"])
    synth.write_read_lib(os.path.join(d, "reads"), [reads])
    k = load_files_into(engine, read2sdbg(d, c, os.path.join(d, "reads")))
    info = engine.sdbg_build_index(k)
    assert info.n_items > 256 * TILE
    want = check_histogram(engine, info)
    assert want[1] > want[2:].sum()  # most edges on one value: the LDS bins take them


def synthetic_stream(n, seed):
    """an SdBG byte stream of n records made with numpy (sdbg_item.h: byte 0 = W | last << 4 | tip << 5, byte 1 = the multiplicity or
    255 = two more bytes hold it), spread over the 65536 buckets; W == 0 makes an edge invalid.  No tips (no labels)."""
    rng = np.random.default_rng(seed)
    byte0 = rng.integers(0, 9, size=n, dtype=np.uint8) | (rng.integers(0, 2, size=n, dtype=np.uint8) << 4)
    mul = rng.integers(1, 6, size=n, dtype=np.uint16)  # most edges on a handful of values ...
    rare = np.nonzero(rng.random(n) < 0.05)[0]  # ... and a tail up to the last bin, on both sides of the LDS range
    mul[rare] = np.minimum(65535, rng.geometric(1 / 3000.0, size=rare.size)).astype(np.uint16)
    mul[rng.integers(0, n, size=50)] = 65535
    mul[rng.integers(0, n, size=50)] = rng.integers(8190, 8194, size=50, dtype=np.uint16)
    mul[rng.integers(0, n, size=50)] = 0
    large = mul >= 255
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(2 + 2 * large.astype(np.int64), out=off[1:])
    data = np.zeros(int(off[-1]), dtype=np.uint8)
    data[off[:-1]] = byte0
    data[off[:-1] + 1] = np.where(large, 255, mul).astype(np.uint8)
    at = off[:-1][large]
    data[at + 2] = (mul[large] & 255).astype(np.uint8)
    data[at + 3] = (mul[large] >> 8).astype(np.uint8)
    items = rng.multinomial(n, np.full(65536, 1 / 65536.0)).astype(np.uint64)
    first = np.zeros(65537, dtype=np.int64)
    np.cumsum(items, out=first[1:])
    large_before = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(large, out=large_before[1:])
    b_large = (large_before[first[1:]] - large_before[first[:-1]]).astype(np.uint64)
    return data, off[first[:-1]].astype(np.uint64), items, np.zeros(65536, dtype=np.uint64), b_large, mul, byte0


def test_histogram_over_several_tiles_per_workgroup_and_between_flushes(engine):
    """18 M records made with numpy: more tiles than workgroups (4 per compute unit), so a workgroup walks several tiles; the same
    with the LDS bins flushed after every tile and after every second one (knob sdbg_hist_flush_tiles) — the path that keeps the
    32-bit bins from wrapping at item counts no test can hold"""
    n = 18 * 1000 * 1000 + 37
    data, b_off, items, tips, large, mul, byte0 = synthetic_stream(n, 11)
    engine.sdbg_load_bytes(data, b_off, items, tips, large)
    info = engine.sdbg_build_index(21)
    assert info.n_items == n and n % 64 != 0 and n // TILE > 4 * 256
    assert np.array_equal(engine.fetch(lib.BUF_SDBG_MUL, np.uint16), mul)
    want = check_histogram(engine, info)
    assert np.array_equal(want, np.bincount(mul[(byte0 & 15) != 0], minlength=65536).astype(np.uint64))
    assert want[8191] > 0 and want[8192] > 0 and want[65535] > 0 and want[0] > 0
    try:
        for tiles in (1, 2):
            engine.set_option("sdbg_hist_flush_tiles", tiles)
            check_histogram(engine, info)
    finally:
        engine.set_option("sdbg_hist_flush_tiles", 65536)
        engine.trim()


def test_a_graph_without_a_valid_edge(engine):
    """one short read is a tip at both ends: after mhx_sdbg_remove_tips nothing is valid; the histogram is empty and the inference
    says so instead of returning a number"""
    reads = np.random.default_rng(5).integers(0, 4, size=(1, 30), dtype=np.uint8)
    info = graph_from_reads(engine, reads, 21, 1)
    depth, converged = engine.sdbg_infer_min_depth(info)  # as loaded: some edges, one value
    assert converged and depth > 0
    engine.sdbg_remove_tips(info, 42)
    want, inv = expected_histogram(engine, info)
    assert inv.all() and want.sum() == 0
    hist, n_valid = engine.sdbg_mul_histogram(info)
    assert n_valid == 0 and not hist.any()
    with pytest.raises(lib.MhxError, match="no valid edge"):
        engine.sdbg_infer_min_depth(info)


def test_histogram_needs_the_index():
    e = lib.Engine(0)  # a handle of its own: the shared one keeps its state for the other tests
    try:
        with pytest.raises(lib.MhxError, match="mhx_sdbg_build_index"):
            e.sdbg_mul_histogram(lib.SdbgIndexInfo())
        reads = np.random.default_rng(8).integers(0, 4, size=(4, 60), dtype=np.uint8)
        info = graph_from_reads(e, reads, 21, 1)
        check_histogram(e, info)
        assert e.lib.mhx_reset(e.h) == 0
        for call in (e.sdbg_mul_histogram, e.sdbg_infer_min_depth):
            with pytest.raises(lib.MhxError, match="mhx_sdbg_build_index"):
                call(info)
    finally:
        e.close()


def test_golden_graphs_equal_the_reference_histogram_and_depth(engine, graph_of):
    """every golden case: the graph of `mhx_core read2sdbg` -> index -> the device histogram = the reference's own, the inferred
    depth prints as the reference logged it"""
    for c in GOLDEN:
        k = load_files_into(engine, graph_of(c))
        info = engine.sdbg_build_index(k)
        assert info.n_items == c["n_items"] and info.n_large == c["n_large"]
        depth, converged = engine.sdbg_infer_min_depth(info)
        hist = engine.fetch(lib.BUF_SDBG_MUL_HIST, np.uint64)
        assert [[int(v), int(hist[v])] for v in np.nonzero(hist)[0]] == c["hist"], c["name"]
        assert converged and "%.3f" % depth == c["log"]["min_depth"], c["name"]
        assert (depth, converged) == lib.infer_min_depth(hist) and info.use_full_mul == c["full_mul"]


def run_assemble(d, g, c, out, exe=None, env_extra=None, route=None, args=None, level="2"):
    """mhx_core assemble with the route's opt-in variable at `level` (2: a missing depth is inferred) and a reference that fails"""
    env = dict(os.environ, MHX_REF_CORE=stub(d))
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE", "MHX_ASSEMBLE_BUBBLE"):
        env.pop(name, None)
    env["MHX_ASSEMBLE_" + (route or c["route"])] = level
    env.update(env_extra or {})
    p = subprocess.run([exe or gu.MHX_CORE, "assemble", "-s", g, "-o", out] + (c["args"] if args is None else args), env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stderr


def check_against_golden(c, out, stderr):
    print(c["name"], [ln for ln in stderr.splitlines() if "min depth" in ln])
    assert mig.parse_log(c["route"], stderr) == c["log"]
    for s, want in c["digests"].items():
        with open(out + s, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want, s


@pytest.mark.parametrize("c", GOLDEN, ids=lambda c: c["name"])
def test_assemble_infers_its_minimum_depth(c, graph_of, tmp_path):
    """(fails before mhx_sdbg_infer_min_depth: such a command line went to MHX_REF_CORE at every level, here the stub that exits with 97)"""
    d = str(tmp_path)
    out = os.path.join(d, "mine")
    check_against_golden(c, out, run_assemble(d, graph_of(c), c, out))


def test_inference_through_the_resident_server(graph_of, tmp_path):
    """the route is decided from argv alone, so the server takes it too"""
    d = str(tmp_path)
    c = BY_NAME["A-orchestrator-p3"]
    out = os.path.join(d, "mine")
    with gu.socket_dir() as sd:
        sock = os.path.join(sd, "s")
        try:
            err = run_assemble(d, graph_of(c), c, out, exe=os.path.join(gu.ROOT, "megahit_amd", "megahit_core"),
                               env_extra={"MHX_SERVER": sock, "MHX_SERVER_AUTOSTART": "1"})
        finally:
            subprocess.run([gu.MHX_CORE, "--serve-stop", sock], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=60)
    check_against_golden(c, out, err)


def test_prune_level_0_neither_infers_nor_logs(graph_of, tmp_path):
    """a command line served before: prune level 0 with the default --min_depth -1 never reads the value"""
    d = str(tmp_path)
    c = CLEAN_GOLDEN["A"]
    assert "--min_depth" not in mcg.assemble_args(c) and mcg.assemble_args(c)[:4] == ["--bubble_level", "0", "--prune_level", "0"]
    out = os.path.join(d, "mine")
    err = run_assemble(d, graph_of(c), c, out, route="CLEAN", args=mcg.assemble_args(c), level="1")
    assert "min depth" not in err and "Cannot detect" not in err
    assert mcg.parse_log(err) == c["log"]
    for s, want in c["digests"].items():
        with open(out + s, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want, s


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")
@pytest.mark.parametrize("name,seed", [("A-p2", 301), ("A-p2", 302), ("A-orchestrator-p3", 303), ("A-orchestrator-p3", 304)])
def test_fresh_seeds_against_the_reference(name, seed, tmp_path):
    d = str(tmp_path)
    c = dict(BY_NAME[name], seed=seed)
    g = read2sdbg(d, c)
    mine, ref = os.path.join(d, "mine"), os.path.join(d, "ref")
    err = run_assemble(d, g, c, mine)
    q = subprocess.run([REF, "assemble", "-s", g, "-o", ref, "-t", "1"] + c["args"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    want = mig.parse_log(c["route"], q.stderr)
    assert want["min_depth"] is not None and mig.parse_log(c["route"], err) == want
    for s in mig.FILES:
        with open(mine + s, "rb") as a, open(ref + s, "rb") as b:
            got, exp = a.read(), b.read()
        assert got == exp, "%s differs (%d vs %d bytes)" % (s, len(got), len(exp))
