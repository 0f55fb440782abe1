"""GPU: bubble popping and prune level 3 of `assemble` on the device (include/mhx.h mhx_unitig_pop_bubbles,
mhx_unitig_remove_low_depth; `mhx_core assemble` with MHX_ASSEMBLE_BUBBLE=1) against the reference's own `megahit_core assemble
-t 1` on the same graph, byte for byte, on fresh seeds, a long genome and through the resident server; the Engine-level calls
against the committed counts; a pop with nothing to pop; a finish in mid-run; the early return of the complex pass; the error
paths.  mhx_core runs with MHX_REF_CORE pointing to a stub that fails loudly, so a run that forwarded cannot pass."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from megahit_amd import canon, lib

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_bubble_golden as mbg  # noqa: E402

pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")
with open(os.path.join(gu.GOLD, "unitig_bubble.json")) as f:
    GOLDEN = {c["name"]: c for c in json.load(f)["cases"]}


def stub(d):
    p = os.path.join(d, "ref_stub.sh")
    with open(p, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(p, 0o755)
    return p


def graph(d, c):
    """the case's library -> mhx_core read2sdbg -> the graph's prefix"""
    out = os.path.join(d, "g")
    subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", mbg.write_library(d, c), "--output_prefix", out] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    return out


def assemble_both(d, g, c, tag="", exe=None, env_extra=None):
    """mhx_core (opted in) and the reference at -t 1 on graph g: every file byte for byte, the logged counts alike"""
    env = dict(os.environ, MHX_REF_CORE=stub(d), MHX_ASSEMBLE_BUBBLE="1")
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE"):
        env.pop(name, None)
    env.update(env_extra or {})
    mine, ref = os.path.join(d, "mine" + tag), os.path.join(d, "ref" + tag)
    args = mbg.assemble_args(c)
    p = subprocess.run([exe or gu.MHX_CORE, "assemble", "-s", g, "-o", mine, "-t", "4"] + args, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([REF, "assemble", "-s", g, "-o", ref, "-t", "1"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    want = mbg.parse_log(q.stderr)
    assert mbg.parse_log(p.stderr) == want
    stat = r"Max: (\d+), Min: (\d+), N50: (\d+), number contigs: (\d+), number isolated: (\d+), number looped: (\d+), total size: (\d+)"
    assert re.findall(stat, p.stderr) == re.findall(stat, q.stderr)
    for s in mbg.FILES:
        assert os.path.exists(mine + s) == os.path.exists(ref + s), s
        if os.path.exists(ref + s):
            with open(mine + s, "rb") as a, open(ref + s, "rb") as b:
                got, exp = a.read(), b.read()
            assert got == exp, "%s differs (%d vs %d bytes)" % (s, len(got), len(exp))
    want["bubble_records"] = mbg.records(ref + ".bubble_seq.fa")
    want["bubble_seq"] = ref + ".bubble_seq.fa"
    return want


FRESH = [
    dict(mbg.A, seed=301, name="A-seed301"),
    dict(mbg.B, seed=302, name="B-seed302"),
    dict(mbg.A, m=1, err=0.02, seed=303, name="A-m1-seed303"),
]


@needs_ref
@pytest.mark.parametrize("lib_", FRESH, ids=lambda c: c["name"])
def test_bubbles_match_reference_on_fresh_seeds(lib_, tmp_path):
    """bubble level 2 with careful records at prune level 2 (non-final), and at prune level 3 in a final round"""
    d = str(tmp_path)
    g = graph(d, lib_)
    a = assemble_both(d, g, dict(lib_, bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=mbg.ORCH))
    assert sum(a["naive"]) > 0 and sum(a["complex"]) > 0 and a["bubble_records"] > 0
    b = assemble_both(d, g, dict(lib_, bubble=2, prune=3, final=True, careful=True, min_depth=2, rounds=5, opts=mbg.ORCH), tag="-p3")
    assert len(b["more_pruned"]) == b["rounds_run"] > 0


@needs_ref
def test_careful_records_of_long_neighbours(tmp_path):
    """a 200 kb genome with a second haplotype: after the first rounds the left and right vertices of a bubble are contigs of
    tens of kb, which the careful records carry whole"""
    d = str(tmp_path)
    c = dict(mbg.A, G=200000, pairs=40000, seed=311, gap=2000, bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=mbg.ORCH)
    want = assemble_both(d, graph(d, c), c)
    assert want["bubble_records"] > 0
    with open(want["bubble_seq"]) as f:
        assert max(int(x) for x in re.findall(r"len=(\d+)", f.read())) > 20000


@needs_ref
def test_bubbles_through_the_resident_server(tmp_path):
    """the request carries MHX_ASSEMBLE_BUBBLE: the route works in the server too"""
    d = str(tmp_path)
    c = dict(mbg.A, seed=304, name="A-seed304", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=mbg.ORCH)
    g = graph(d, c)
    with gu.socket_dir() as sd:
        sock = os.path.join(sd, "s")
        exe = os.path.join(gu.ROOT, "megahit_amd", "megahit_core")
        try:
            assemble_both(d, g, c, exe=exe, env_extra={"MHX_SERVER": sock, "MHX_SERVER_AUTOSTART": "1"})
        finally:
            subprocess.run([gu.MHX_CORE, "--serve-stop", sock], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=60)


def load_files_into(engine, prefix):
    hdr, buckets = canon.canonical_sdbg(prefix)
    off = np.zeros(65536, dtype=np.uint64)
    items, tips, large = off.copy(), off.copy(), off.copy()
    parts, pos = [], 0
    for bid, ni, nt, nl, b in buckets:
        off[bid], items[bid], tips[bid], large[bid] = pos, ni, nt, nl
        parts.append(b)
        pos += len(b)
    data = np.frombuffer(b"".join(parts), dtype=np.uint8) if parts else np.zeros(0, dtype=np.uint8)
    engine.sdbg_load_bytes(data, off, items, tips, large)
    return hdr["k"]


def fresh_unitigs(engine, prefix):
    """graph files -> index, SdBG-level tips, unitig graph; returns (k, info)"""
    k = load_files_into(engine, prefix)
    info = engine.sdbg_build_index(k)
    engine.sdbg_remove_tips(info, 2 * k)
    engine.sdbg_unitigs(info)
    return k, info


def table(engine):
    return engine.fetch(lib.BUF_UNITIG_VERTICES, np.uint8).view(lib.UNITIG_VERTEX_DTYPE).copy()


def complex_max_len(k, merge_len=20, sim=0.95):
    return int(round(merge_len * k / sim))  # lround of a positive number that is no half-integer here


def rounds(engine, info, k, c, finish_in_between=False, careful=-1.0):
    """main_assemble.cpp:182-249 at bubble level 2 and prune level 2 through the Engine; returns the counts as parse_log names
    them, and all the careful records"""
    got = dict(disconnected=[], tips=[], pruned=[], naive=[], complex=[])
    recs = []
    for rnd in range(1, c["rounds"] + 1):
        changed = False
        if rnd > 1:
            got["tips"].append(engine.unitig_remove_tips(info, 2 * k))
            changed |= got["tips"][-1] > 0
        n, r = engine.unitig_pop_bubbles(info, k + 2, 0.0, careful)
        assert r == len(engine.unitig_bubble_records())
        recs += engine.unitig_bubble_records()
        got["naive"].append(n)
        if finish_in_between:
            engine.unitig_finish(info)
        n2, r = engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95, careful)
        recs += engine.unitig_bubble_records()
        got["complex"].append(n2)
        changed |= n > 0 or n2 > 0
        got["disconnected"].append(engine.unitig_disconnect_weak_links(info, 0.1))
        changed |= got["disconnected"][-1] > 0
        if finish_in_between:
            engine.unitig_finish(info)
        got["pruned"].append(engine.unitig_remove_local_low_depth(info, c["min_depth"], 2 * k, 1000, 0.1, False)[0])
        if not changed:
            break
    return got, recs


def test_engine_calls_reproduce_the_committed_counts(engine, tmp_path):
    """case A-b2-careful pass by pass, with and without a finish between the pops: the same counts, records, table and text"""
    c = GOLDEN["A-b2-careful"]
    g = graph(str(tmp_path), c)
    results = []
    for between in (False, True):
        k, info = fresh_unitigs(engine, g)
        got, recs = rounds(engine, info, k, c, finish_in_between=between, careful=0.2)
        for key in ("naive", "complex", "disconnected", "tips", "pruned"):
            assert got[key] == c["log"][key], key
        assert engine.unitig_iterate_local_low_depth(info, c["min_depth"], 2 * k, 1000, 0.2, True) == c["log"]["final_pass"][0]
        n, r = engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95, -1.0, True)  # the final pop: marks, no records
        assert (n, r) == (c["log"]["final_pass"][1], 0) and engine.unitig_bubble_records() == []
        assert len(recs) == c["log"]["bubble_records"]
        res = engine.unitig_finish(info)
        v, text = engine.unitig_contigs()
        assert (res.n_vertices, res.n_standalone, res.n_loops) == (c["log"]["final"]["contigs"], c["log"]["final"]["isolated"], c["log"]["final"]["looped"])
        assert int(((v["flags"] & lib.UNITIG_CHANGED) != 0).sum()) == c["log"]["addi_records"]
        results.append((v.copy(), text, recs))
    a, b = results
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def test_records_are_the_vertices_before_the_refresh(engine, tmp_path):
    """the first naive pop of case A-b1-careful-p0: every record is the text and the average depth of its vertex in the table
    the pass ran on, a bubble's records end with its left and right vertex, and the deleted middles are gone afterwards"""
    c = GOLDEN["A-b1-careful-p0"]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    v, text = engine.unitig_contigs()
    n, r = engine.unitig_pop_bubbles(info, k + 2, 0.0, 0.2)
    recs = engine.unitig_bubble_records()
    assert n == c["log"]["naive"][0] and r == len(recs) > 0
    for seq, depth, vid in recs:
        assert seq == text[vid] and depth == float(v["total_depth"][vid]) / float(v["length"][vid])
    assert engine.unitig_bubble_stats() == dict(candidates=0, passed=0, failed=0, finishes=0)  # the text of mhx_sdbg_unitigs was still good
    assert table(engine).size < v.size
    n2, r2 = engine.unitig_pop_bubbles(info, k + 2, 0.0, 0.2)
    assert engine.unitig_bubble_stats()["finishes"] == (1 if r2 else 0)  # a Refresh ran since: records need a finish first


def test_nothing_to_pop_and_the_early_return_leave_the_table_alone(engine, tmp_path):
    """max_len = 0: no middle is short enough; max_len * (1 - similarity) < 1: the complex pass returns before its Refresh —
    the vertex table stays bit for bit and no MHX_UNITIG_CHANGED appears although the calls ask for marks"""
    c = GOLDEN["A-b2"]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    before = table(engine)
    assert engine.unitig_pop_bubbles(info, 0, 0.0, 0.2, True) == (0, 0)
    assert engine.unitig_pop_bubbles(info, 0, 0.95, 0.2, True) == (0, 0)
    assert engine.unitig_pop_bubbles(info, 19, 0.95, 0.2, True) == (0, 0)   # 19 * 0.05 < 1, whatever the graph holds
    assert engine.unitig_pop_bubbles(info, 21, 0.99, -1.0, True) == (0, 0)  # lround(1 * 21 / 0.99) = 21: --merge_len 1 --merge_similar 0.99
    assert engine.unitig_remove_low_depth(info, 0.0) == 0
    after = table(engine)
    assert np.array_equal(before, after) and not (after["flags"] & lib.UNITIG_CHANGED).any()
    assert engine.unitig_pop_bubbles(info, k + 2, 0.0, -1.0, True)[0] == c["log"]["naive"][0]  # and the graph still pops as committed
    with pytest.raises(lib.MhxError, match="cap"):
        engine.unitig_pop_bubbles(info, lib.SIM_MAX_LEN, 0.95)  # max_len + k is beyond the cap: an error, not a guess


def test_remove_low_depth_matches_the_committed_count(engine, tmp_path):
    """case C-b2-m1-p3, round 1 up to RemoveLowDepth and its two pops: the (more-)excessive count"""
    c = GOLDEN["C-b2-m1-p3"]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    assert engine.unitig_pop_bubbles(info, k + 2)[0] == c["log"]["naive"][0]
    assert engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95)[0] == c["log"]["complex"][0]
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][0]
    n = engine.unitig_remove_low_depth(info, c["min_depth"])
    assert n > 0
    n += engine.unitig_pop_bubbles(info, k + 2)[0]
    n += engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95)[0]
    assert n == c["log"]["more_pruned"][0]


def test_popping_needs_the_unitig_graph_of_this_index(tmp_path):
    """the new calls before mhx_sdbg_unitigs, after mhx_trim, after a new SdBG-level trimming or a new index: the "run
    mhx_sdbg_unitigs first" error"""
    engine = lib.Engine(0)  # a handle of its own: the shared one keeps its state for the other tests
    try:
        c = dict(mbg.A, G=3000, pairs=600)
        g = graph(str(tmp_path), c)
        k = load_files_into(engine, g)
        info = engine.sdbg_build_index(k)

        def all_fail():
            for call in (lambda: engine.unitig_pop_bubbles(info, k + 2), lambda: engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95, 0.2),
                         lambda: engine.unitig_remove_low_depth(info, 2)):
                with pytest.raises(lib.MhxError, match="mhx_sdbg_unitigs"):
                    call()

        all_fail()  # no unitig graph yet
        assert engine.unitig_similarity("ACGTACGTACGTACGTACGTACGT", "ACGTACGTACGTACGAACGTACGT", 0.95) > 0.95  # needs no graph
        engine.sdbg_unitigs(info)
        engine.unitig_pop_bubbles(info, k + 2)
        engine.trim()
        all_fail()
        engine.sdbg_unitigs(info)
        engine.unitig_pop_bubbles(info, complex_max_len(k), 0.95, 0.2)
        engine.sdbg_remove_tips(info, 2 * k)  # a new trimming of the SdBG
        all_fail()
        engine.sdbg_unitigs(info)
        info = engine.sdbg_build_index(k)  # a new index
        all_fail()
    finally:
        engine.close()
