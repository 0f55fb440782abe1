"""GPU: the cleaning rounds of `assemble` on the device (include/mhx.h mhx_unitig_disconnect_weak_links,
mhx_unitig_remove_tips, mhx_unitig_finish; `mhx_core assemble` with MHX_ASSEMBLE_CLEAN=1) against the reference's own
`megahit_core assemble -t 1` on the same graph, byte for byte, on fresh seeds, a long genome and through the resident
server; the Engine-level calls against the committed counts; the error paths.  mhx_core runs with MHX_REF_CORE pointing to a
stub that fails loudly, so a run that forwarded instead of computing cannot pass."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from megahit_amd import canon, lib, synth

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_clean_golden as mcg  # noqa: E402

pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")


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


def assemble_both(d, g, c, exe=None, env_extra=None):
    """mhx_core (opted in) and the reference at -t 1 on graph g: the six files byte for byte, the logged counts alike"""
    env = dict(os.environ, MHX_REF_CORE=stub(d), MHX_ASSEMBLE_CLEAN="1")
    env.pop("MHX_SERVER", None)
    env.pop("MHX_ASSEMBLE_REF", None)
    env.update(env_extra or {})
    mine, ref = os.path.join(d, "mine"), os.path.join(d, "ref")
    args = mcg.assemble_args(c)
    p = subprocess.run([exe or gu.MHX_CORE, "assemble", "-s", g, "-o", mine, "-t", "4"] + args, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([REF, "assemble", "-s", g, "-o", ref, "-t", "1"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    want = mcg.parse_log(q.stderr)
    assert mcg.parse_log(p.stderr) == want
    assert re.findall(r"Max: (\d+), Min: (\d+), N50: (\d+)", p.stderr) == re.findall(r"Max: (\d+), Min: (\d+), N50: (\d+)", q.stderr)
    for s in mcg.FILES:
        with open(mine + s, "rb") as a, open(ref + s, "rb") as b:
            got, exp = a.read(), b.read()
        assert got == exp, "%s differs (%d vs %d bytes)" % (s, len(got), len(exp))
    want["ref_log"] = q.stderr
    return want


FRESH = [
    dict(mcg.A, seed=101, name="A-seed101", rounds=5, opts=[]),
    dict(mcg.A, seed=102, name="A-seed102", rounds=5, opts=[]),
    dict(mcg.C, seed=103, name="C-seed103", rounds=5, opts=[]),
]


@needs_ref
@pytest.mark.parametrize("c", FRESH, ids=lambda c: c["name"])
def test_cleaning_matches_reference_on_fresh_seeds(c, tmp_path):
    d = str(tmp_path)
    want = assemble_both(d, graph(d, c), c)
    assert want["disconnected"][0] > 0


@needs_ref
def test_cleaning_merges_long_paths(tmp_path):
    """200 kb at 1 % errors and 80 x coverage: no unitig is longer than a few hundred bases before cleaning; Refresh merges paths
    of hundreds of vertices into contigs of tens of kb and more, by pointer jumping"""
    d = str(tmp_path)
    c = dict(kind="linear", G=200000, pairs=80000, err=0.01, seed=111, read_len=100, frag=250, k=21, m=2, mercy=False, rounds=5, opts=[])
    want = assemble_both(d, graph(d, c), c)
    assert want["disconnected"][0] > 0 and sum(want["tips"]) > 0
    longest = [int(x) for x in re.findall(r"Max: (\d+)", want["ref_log"])]  # the reference's statistics before and after cleaning
    assert longest[0] < 2000 and longest[-1] > 20000


@needs_ref
def test_cleaning_through_the_resident_server(tmp_path):
    """the request carries MHX_ASSEMBLE_CLEAN: the route works in the server too"""
    d = str(tmp_path)
    c = dict(mcg.A, seed=104, name="A-seed104", rounds=5, opts=["--disconnect_ratio", "0.2"])
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


def test_engine_calls_match_the_committed_counts(engine, tmp_path):
    """case A step by step: weak links, tips, weak links, finish"""
    with open(os.path.join(gu.GOLD, "unitig_clean.json")) as f:
        c = [x for x in json.load(f)["cases"] if x["name"] == "A"][0]
    k = load_files_into(engine, graph(str(tmp_path), c))
    info = engine.sdbg_build_index(k)
    engine.sdbg_remove_tips(info, 2 * k)
    r = engine.sdbg_unitigs(info)
    assert r.n_vertices == c["log"]["graph_size"]
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][0]
    assert engine.unitig_remove_tips(info, 2 * k) == c["log"]["tips"][0]
    assert engine.unitig_disconnect_weak_links(info, 0.1) == c["log"]["disconnected"][1]
    r = engine.unitig_finish(info)
    assert (r.n_vertices, r.n_standalone, r.n_loops) == (c["log"]["final"]["contigs"], c["log"]["final"]["isolated"], c["log"]["final"]["looped"])
    v, text = engine.unitig_contigs()
    assert v.size == r.n_vertices and sum(map(len, text)) == r.n_bases
    assert (v["length"] > 0).all()
    assert all(len(t) == k + n for t, n in zip(text, v["length"]))
    assert all(set(t) <= set("ACGT") for t in text)
    assert np.unique(v["b"]).size == v.size


def test_cleaning_before_unitigs_is_an_error(engine, tmp_path):
    """each entry needs the unitig graph of the current index: anything else is an error, not a fault"""
    c = dict(mcg.A, G=3000, pairs=600)
    k = load_files_into(engine, graph(str(tmp_path), c))
    info = engine.sdbg_build_index(k)
    for call in (lambda: engine.unitig_disconnect_weak_links(info, 0.1), lambda: engine.unitig_remove_tips(info, 2 * k),
                 lambda: engine.unitig_finish(info)):
        with pytest.raises(lib.MhxError, match="mhx_sdbg_unitigs"):
            call()
    engine.sdbg_unitigs(info)
    engine.unitig_disconnect_weak_links(info, 0.1)
    # a new index drops the graph again
    info = engine.sdbg_build_index(k)
    with pytest.raises(lib.MhxError, match="mhx_sdbg_unitigs"):
        engine.unitig_finish(info)


def test_trim_and_reset_drop_the_unitig_graph(tmp_path):
    """trim() frees the workspaces the cleaning state lives in, mhx_reset forgets the vertex table: a cleaning call after either
    is the same clear error, not a read of memory that is gone"""
    engine = lib.Engine(0)  # a handle of its own: the shared one keeps its state for the other tests
    try:
        c = dict(mcg.A, G=3000, pairs=600)
        k = load_files_into(engine, graph(str(tmp_path), c))
        info = engine.sdbg_build_index(k)
        engine.sdbg_unitigs(info)
        engine.trim()
        with pytest.raises(lib.MhxError, match="mhx_sdbg_unitigs"):
            engine.unitig_disconnect_weak_links(info, 0.1)
        engine.sdbg_unitigs(info)
        engine.unitig_disconnect_weak_links(info, 0.1)
        engine.trim()  # between two cleaning calls: the owner map and the flags are gone
        for call in (lambda: engine.unitig_remove_tips(info, 2 * k), lambda: engine.unitig_finish(info)):
            with pytest.raises(lib.MhxError, match="mhx_sdbg_unitigs"):
                call()
        engine.sdbg_unitigs(info)
        assert engine.lib.mhx_reset(engine.h) == 0
        with pytest.raises(lib.MhxError):
            engine.unitig_disconnect_weak_links(info, 0.1)
    finally:
        engine.close()


def test_cleaning_a_graph_without_valid_edges(tmp_path):
    """a few short reads at m = 1: every path goes as a tip; the cleaning rounds run on nothing -> empty outputs"""
    d = str(tmp_path)
    rng = np.random.default_rng(11)
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [rng.integers(0, 4, size=(6, 40), dtype=np.uint8)], paired=False)
    g = os.path.join(d, "g")
    subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", "21", "-m", "1", "--host_mem", "2e9", "--num_cpu_threads", "4", "--read_lib_file", prefix,
                    "--output_prefix", g], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    env = dict(os.environ, MHX_REF_CORE=stub(d), MHX_ASSEMBLE_CLEAN="1")
    env.pop("MHX_SERVER", None)
    env.pop("MHX_ASSEMBLE_REF", None)
    out = os.path.join(d, "mine")
    p = subprocess.run([gu.MHX_CORE, "assemble", "-s", g, "-o", out, "--bubble_level", "0", "--prune_level", "0"], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Number unitigs disconnected: 0" in p.stderr
    for s in (".contigs.fa", ".final.contigs.fa", ".bubble_seq.fa"):
        assert os.path.getsize(out + s) == 0
        with open(out + s + ".info") as f:
            assert f.read() == "0 0\n"
