"""GPU: the low-depth pruning of `assemble` on the device (include/mhx.h mhx_unitig_remove_local_low_depth,
mhx_unitig_iterate_local_low_depth, MHX_UNITIG_CHANGED; `mhx_core assemble` with MHX_ASSEMBLE_PRUNE=1) against the reference's
own `megahit_core assemble -t 1` on the same graph, byte for byte, on fresh seeds, a long genome and through the resident
server; the Engine-level calls against the committed counts; a finish in mid-run; the error paths.  mhx_core runs with
MHX_REF_CORE pointing to a stub that fails loudly, so a run that forwarded instead of computing cannot pass."""
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
import make_unitig_prune_golden as mpg  # noqa: E402

mcg = mpg.mcg
pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")
with open(os.path.join(gu.GOLD, "unitig_prune.json")) as f:
    GOLDEN = {c["name"]: c for c in json.load(f)["cases"]}
with open(os.path.join(gu.GOLD, "unitig_clean.json")) as f:
    CLEAN_GOLDEN = {c["name"]: c for c in json.load(f)["cases"]}
LOCAL_WIDTH = 1000


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
                    "--read_lib_file", mcg.write_library(d, c), "--output_prefix", out] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    return out


def assemble_both(d, g, c, tag="", exe=None, env_extra=None):
    """mhx_core (opted in) and the reference at -t 1 on graph g: the eight files byte for byte, the logged counts alike"""
    env = dict(os.environ, MHX_REF_CORE=stub(d), MHX_ASSEMBLE_PRUNE="1")
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN"):
        env.pop(name, None)
    env.update(env_extra or {})
    mine, ref = os.path.join(d, "mine" + tag), os.path.join(d, "ref" + tag)
    args = mpg.assemble_args(c)
    p = subprocess.run([exe or gu.MHX_CORE, "assemble", "-s", g, "-o", mine, "-t", "4"] + args, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([REF, "assemble", "-s", g, "-o", ref, "-t", "1"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    want = mpg.parse_log(q.stderr)
    assert mpg.parse_log(p.stderr) == want
    stat = r"Max: (\d+), Min: (\d+), N50: (\d+), number contigs: (\d+), number isolated: (\d+), number looped: (\d+), total size: (\d+)"
    assert re.findall(stat, p.stderr) == re.findall(stat, q.stderr)
    for s in mpg.FILES:
        with open(mine + s, "rb") as a, open(ref + s, "rb") as b:
            got, exp = a.read(), b.read()
        assert got == exp, "%s differs (%d vs %d bytes)" % (s, len(got), len(exp))
    want["addi_records"] = mpg.addi_records(ref)
    want["ref_log"] = q.stderr
    return want


FRESH = [
    dict(mcg.A, seed=201, name="A-seed201"),
    dict(mcg.B, seed=202, name="B-seed202"),
    dict(mcg.C, pairs=1500, err=0.02, seed=203, name="C-seed203"),
]


@needs_ref
@pytest.mark.parametrize("lib_", FRESH, ids=lambda c: c["name"])
def test_pruning_matches_reference_on_fresh_seeds(lib_, tmp_path):
    """two linear graphs and a circular one at prune level 2, non-final (.addi.fa) and final (one output, after the iteration)"""
    d = str(tmp_path)
    g = graph(d, lib_)
    for final in (False, True):
        c = dict(lib_, prune=2, final=final, min_depth=2, rounds=5, opts=[])
        want = assemble_both(d, g, c, tag="-final" if final else "")
        assert want["rounds_run"] > 0 and len(want["pruned"]) == want["rounds_run"]


@needs_ref
def test_pruning_next_to_long_neighbours(tmp_path):
    """200 kb at 1 % errors and 80 x coverage: after the rounds the contigs are tens of kb long, so the candidates of the
    iteration have neighbours longer than local_width, which count with average depth * local_width"""
    d = str(tmp_path)
    c = dict(kind="linear", G=200000, pairs=80000, err=0.01, seed=111, read_len=100, frag=250, k=21, m=2, mercy=False, prune=2, final=False,
             min_depth=2, rounds=5, opts=[])
    want = assemble_both(d, graph(d, c), c)
    log = want["ref_log"]
    before = log[:log.index("Number of local low depth unitigs removed")]
    assert max(int(x) for x in re.findall(r"Max: (\d+)", before)) > 20000
    assert want["low_depth_removed"] > 0


@needs_ref
def test_pruning_through_the_resident_server(tmp_path):
    """the request carries MHX_ASSEMBLE_PRUNE: the route works in the server too"""
    d = str(tmp_path)
    c = dict(mcg.B, seed=204, name="B-seed204", prune=2, final=False, min_depth=2, rounds=5, opts=["--disconnect_ratio", "0.05"])
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


def rounds(engine, info, k, c, finish_in_between=False):
    """main_assemble.cpp:182-249 at bubble level 0 through the Engine; returns the counts as parse_log names them"""
    got = dict(disconnected=[], tips=[], pruned=[])
    for rnd in range(1, c["rounds"] + 1):
        changed = False
        if rnd > 1:
            got["tips"].append(engine.unitig_remove_tips(info, 2 * k))
            changed |= got["tips"][-1] > 0
        got["disconnected"].append(engine.unitig_disconnect_weak_links(info, 0.1))
        changed |= got["disconnected"][-1] > 0
        if finish_in_between:
            engine.unitig_finish(info)
        if c["prune"] >= 2:
            got["pruned"].append(engine.unitig_remove_local_low_depth(info, c["min_depth"], 2 * k, LOCAL_WIDTH, 0.1, False)[0])
        if not changed:
            break
    return got


@pytest.mark.parametrize("name", ["A-p2", "B-m1"])
def test_single_pass_matches_the_committed_first_round(engine, tmp_path, name):
    c = GOLDEN[name]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][0]
    n, changed = engine.unitig_remove_local_low_depth(info, c["min_depth"], 2 * k, LOCAL_WIDTH, 0.1, False)
    assert n == c["log"]["pruned"][0]
    # the reference does not log its return value; whenever something was deleted it is true
    assert changed or n == 0
    if name == "B-m1":
        assert n > 0 and changed is True
    # the same pass once more on the refreshed graph: what was below the threshold is gone
    n2, _ = engine.unitig_remove_local_low_depth(info, c["min_depth"], 2 * k, LOCAL_WIDTH, 0.1, False)
    assert n2 <= n
    v, _ = (engine.unitig_finish(info), engine.unitig_contigs())[1]
    assert not (v["flags"] & lib.UNITIG_CHANGED).any()


def test_iterate_and_changed_flags_match_the_committed_counts(engine, tmp_path):
    """case A-p2 through the Engine: the iteration's total, MHX_UNITIG_CHANGED on as many vertices as .addi.fa has records —
    and on none without mark_changed, with the same graph otherwise"""
    c = GOLDEN["A-p2"]
    g = graph(str(tmp_path), c)
    tables = []
    for mark in (True, False):
        k, info = fresh_unitigs(engine, g)
        got = rounds(engine, info, k, c)
        assert (got["disconnected"], got["tips"], got["pruned"]) == (c["log"]["disconnected"], c["log"]["tips"], c["log"]["pruned"])
        assert engine.unitig_iterate_local_low_depth(info, c["min_depth"], 2 * k, LOCAL_WIDTH, 0.2, mark) == c["log"]["low_depth_removed"]
        r = engine.unitig_finish(info)
        assert (r.n_vertices, r.n_standalone, r.n_loops) == (c["log"]["final"]["contigs"], c["log"]["final"]["isolated"], c["log"]["final"]["looped"])
        v, text = engine.unitig_contigs()
        assert int(((v["flags"] & lib.UNITIG_CHANGED) != 0).sum()) == (c["log"]["addi_records"] if mark else 0)
        tables.append((v.copy(), text))
    a, b = tables
    a[0]["flags"] &= ~np.uint32(lib.UNITIG_CHANGED)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_finish_in_mid_run_changes_nothing(engine, tmp_path):
    """B-m1 (the rounds prune, the iteration marks): a finish after every weak-link step and before the iteration, then more
    cleaning and the last finish, gives the vertex table and text of the same calls without those finishes"""
    c = GOLDEN["B-m1"]
    g = graph(str(tmp_path), c)
    results = []
    for between in (False, True):
        k, info = fresh_unitigs(engine, g)
        if between:
            engine.unitig_finish(info)  # straight after mhx_sdbg_unitigs: the owner map comes from the first ranking
        got = rounds(engine, info, k, c, finish_in_between=between)
        assert got["pruned"] == c["log"]["pruned"]
        if between:
            engine.unitig_finish(info)
        assert engine.unitig_iterate_local_low_depth(info, c["min_depth"], 2 * k, LOCAL_WIDTH, 0.2, True) == c["log"]["low_depth_removed"]
        r = engine.unitig_finish(info)
        v, text = engine.unitig_contigs()
        results.append((r.n_vertices, r.n_standalone, r.n_loops, r.n_bases, v.copy(), text))
    a, b = results
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4]) and a[5] == b[5]
    assert int(((a[4]["flags"] & lib.UNITIG_CHANGED) != 0).sum()) == c["log"]["addi_records"]


def test_the_old_route_sets_no_new_flag(engine, tmp_path):
    """weak links and tips as tests/golden/unitig_clean.json has them (case A), flags unmasked: nothing of the pruning leaks in"""
    c = CLEAN_GOLDEN["A"]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][0]
    assert engine.unitig_remove_tips(info, 2 * k) == c["log"]["tips"][0]
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][1]
    r = engine.unitig_finish(info)
    assert (r.n_vertices, r.n_standalone, r.n_loops) == (c["log"]["final"]["contigs"], c["log"]["final"]["isolated"], c["log"]["final"]["looped"])
    v, _ = engine.unitig_contigs()
    assert not (v["flags"] & ~np.uint32(lib.UNITIG_LOOP | lib.UNITIG_PALINDROME | lib.UNITIG_STANDALONE)).any()


def test_nothing_qualifies_at_max_len_0_and_ratio_0_adds_nothing(engine, tmp_path):
    """max_len = 0: no vertex is short enough.  local_ratio = 0: the threshold is min(min_depth, 0 * mean) = 0, no depth is below
    it, and min_depth < 0 never holds: nothing deleted, nothing changed"""
    c = GOLDEN["B-m1"]
    k, info = fresh_unitigs(engine, graph(str(tmp_path), c))
    before = engine.unitig_contigs()[0].copy()
    assert engine.unitig_remove_local_low_depth(info, 1000.0, 0, LOCAL_WIDTH, 0.1, True) == (0, False)
    assert engine.unitig_iterate_local_low_depth(info, 1000.0, 0, LOCAL_WIDTH, 0.2, True) == 0
    assert engine.unitig_remove_local_low_depth(info, 1000.0, 2 * k, LOCAL_WIDTH, 0.0, True) == (0, False)
    assert engine.unitig_iterate_local_low_depth(info, 1000.0, 2 * k, LOCAL_WIDTH, 0.0, True) == 0
    assert np.array_equal(engine.fetch(lib.BUF_UNITIG_VERTICES, np.uint8).view(lib.UNITIG_VERTEX_DTYPE), before)


def test_pruning_needs_the_unitig_graph_of_this_index(tmp_path):
    """both calls after mhx_trim, mhx_reset, a new index or a new SdBG-level trimming: the "run mhx_sdbg_unitigs first" error"""
    engine = lib.Engine(0)  # a handle of its own: the shared one keeps its state for the other tests
    try:
        c = dict(mcg.A, G=3000, pairs=600)
        g = graph(str(tmp_path), c)
        k = load_files_into(engine, g)
        info = engine.sdbg_build_index(k)

        def both_fail(match="mhx_sdbg_unitigs"):
            for call in (lambda: engine.unitig_remove_local_low_depth(info, 2, 2 * k), lambda: engine.unitig_iterate_local_low_depth(info, 2, 2 * k)):
                with pytest.raises(lib.MhxError, match=match):
                    call()

        both_fail()  # no unitig graph yet
        engine.sdbg_unitigs(info)
        engine.unitig_remove_local_low_depth(info, 2, 2 * k)
        engine.trim()
        both_fail()
        engine.sdbg_unitigs(info)
        engine.unitig_iterate_local_low_depth(info, 2, 2 * k)
        engine.sdbg_remove_tips(info, 2 * k)  # a new trimming of the SdBG
        both_fail()
        engine.sdbg_unitigs(info)
        info = engine.sdbg_build_index(k)  # a new index
        both_fail()
        engine.sdbg_unitigs(info)
        assert engine.lib.mhx_reset(engine.h) == 0
        both_fail(match=None)
    finally:
        engine.close()
