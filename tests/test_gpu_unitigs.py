"""GPU: `mhx_core assemble --bubble_level 0 --prune_level 0 --cleaning_rounds 0` (tips, unitig graph, contig output on the
device: include/mhx.h mhx_sdbg_unitigs) against the reference's own `megahit_core assemble -t 1` on the same graph —
byte-identical .contigs.fa, .final.contigs.fa, .bubble_seq.fa and their .info files — and Engine.sdbg_unitigs's counts
against the reference's log.  Graphs come from `mhx_core read2sdbg` on synthetic libraries.  mhx_core runs with
MHX_REF_CORE pointing to a stub that fails loudly, so a run that forwarded instead of computing cannot pass."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
from megahit_amd import canon, lib, synth

pytestmark = pytest.mark.gpu

REF = os.path.join(gu.ROOT, "oracle", "_ref", "ref_megahit_core")
QUAL = ["--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"]
OUTS = [".contigs.fa", ".final.contigs.fa", ".bubble_seq.fa"]

needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_megahit_core not built")


def revcomp(g):
    return (3 - g)[::-1]


def genome(kind, G, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=G, dtype=np.uint8)
    if kind == "palindrome":
        return np.concatenate([g, revcomp(g)])
    return g


def library(d, kind, G=20000, pairs=4000, err=0.01, seed=5, read_len=100, frag=250):
    """reads of a linear / circular / S + revcomp(S) genome -> <d>/reads.{bin,lib_info}"""
    g = genome(kind, G, seed)
    if kind == "circular":
        g = np.concatenate([g, g[:frag + read_len]])  # every window, the ones across the origin included
    reads = synth.gen_pe_reads(pairs, g.size, read_len=read_len, frag=frag, err=err, seed=seed + 1, genome=g)
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [reads])
    return prefix


def stub(d):
    p = os.path.join(d, "ref_stub.sh")
    with open(p, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(p, 0o755)
    return p


def graph(d, lib_prefix, k, mercy=False, m=2):
    out = os.path.join(d, "g")
    args = [gu.MHX_CORE, "read2sdbg", "-k", str(k), "-m", str(m), "--host_mem", "2e9", "--num_cpu_threads", "4", "--read_lib_file", lib_prefix,
            "--output_prefix", out] + (["--need_mercy"] if mercy else [])
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    return out


def assemble_both(d, g, opts, exe=None, env_extra=None):
    env = dict(os.environ, MHX_REF_CORE=stub(d))
    env.pop("MHX_SERVER", None)
    env.update(env_extra or {})
    mine, ref = os.path.join(d, "mine"), os.path.join(d, "ref")
    p = subprocess.run([exe or gu.MHX_CORE, "assemble", "-s", g, "-o", mine] + QUAL + opts, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([REF, "assemble", "-s", g, "-o", ref, "-t", "1"] + QUAL + opts, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    for suf in OUTS:
        for s in (suf, suf + ".info"):
            with open(mine + s, "rb") as a, open(ref + s, "rb") as b:
                got, want = a.read(), b.read()
            assert got == want, "%s differs (%d vs %d bytes)" % (s, len(got), len(want))
    return p.stderr, q.stderr


CASES = [  # (id, library kwargs, k, mercy, assemble options)
    ("k21-linear", dict(kind="linear"), 21, False, []),
    ("k21-mercy", dict(kind="linear"), 21, True, []),
    ("k29-tip0", dict(kind="linear", seed=7), 29, False, ["--max_tip_len", "0"]),
    ("k29-tip10-standalone0", dict(kind="linear", seed=8), 29, False, ["--max_tip_len", "10", "--output_standalone", "--min_standalone", "0"]),
    ("k79-standalone200", dict(kind="linear", seed=9, read_len=150, frag=300), 79, False, ["--output_standalone", "--min_standalone", "200"]),
    ("k21-circular", dict(kind="circular", G=8000, pairs=3000, err=0.0), 21, False, []),
    ("k31-circular-errors-standalone", dict(kind="circular", G=8000, pairs=3000, err=0.005), 31, False, ["--output_standalone", "--min_standalone", "0"]),
    ("k21-palindrome", dict(kind="palindrome", G=6000, pairs=3000, err=0.0), 21, False, []),
    ("k25-palindrome-errors", dict(kind="palindrome", G=6000, pairs=3000, err=0.01), 25, True, ["--output_standalone", "--min_standalone", "0"]),
    ("k21-deep", dict(kind="linear", G=3000, pairs=6000, err=0.002), 21, False, ["--max_tip_len", "-1"]),
]


@needs_ref
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_assemble_matches_reference(case, tmp_path):
    _, kw, k, mercy, opts = case
    d = str(tmp_path)
    g = graph(d, library(d, **kw), k, mercy)
    assemble_both(d, g, opts)


@needs_ref
def test_assemble_no_valid_edge(tmp_path):
    """a few short reads at m = 1: every path is shorter than 2k and goes as a tip -> empty outputs, `0 0` .info files"""
    d = str(tmp_path)
    rng = np.random.default_rng(11)
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [rng.integers(0, 4, size=(6, 40), dtype=np.uint8)], paired=False)
    g = graph(d, prefix, 21, m=1)
    assemble_both(d, g, [])
    with open(os.path.join(d, "mine.contigs.fa.info")) as f:
        assert f.read() == "0 0\n"


@needs_ref
def test_assemble_long_error_free_genome(tmp_path):
    """1 Mb without errors: one unitig of ~10^6 edges (per strand) ranked without a serial walk"""
    d = str(tmp_path)
    g = graph(d, library(d, "linear", G=1_000_000, pairs=60000, err=0.0, seed=21, read_len=150, frag=400), 31)
    assemble_both(d, g, [])
    with open(os.path.join(d, "mine.contigs.fa")) as f:
        lens = [int(re.search(r"len=(\d+)", l).group(1)) for l in f if l.startswith(">")]
    assert max(lens) > 500_000


@needs_ref
def test_assemble_through_the_resident_server(tmp_path):
    """under the reference's name the resident server is the default: the route works in the server too"""
    d = str(tmp_path)
    g = graph(d, library(d, "linear", seed=13), 21)
    with gu.socket_dir() as sd:
        sock = os.path.join(sd, "s")
        exe = os.path.join(gu.ROOT, "megahit_amd", "megahit_core")
        try:
            assemble_both(d, g, ["--max_tip_len", "10"], exe=exe, env_extra={"MHX_SERVER": sock, "MHX_SERVER_AUTOSTART": "1"})
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


@needs_ref
@pytest.mark.parametrize("kind", ["linear", "circular", "palindrome"])
def test_engine_counts_match_reference_log(engine, kind, tmp_path):
    d = str(tmp_path)
    g = graph(d, library(d, kind, G=6000, pairs=3000, err=0.005, seed=17), 21)
    _, log = assemble_both(d, g, [])
    k = load_files_into(engine, g)
    info = engine.sdbg_build_index(k)
    engine.sdbg_remove_tips(info, 2 * k)
    r = engine.sdbg_unitigs(info)
    no_loops, pal = map(int, re.search(r"Graph size without loops: (\d+), palindrome: (\d+)", log).groups())
    assert (r.n_vertices - r.n_loops, r.n_palindromes) == (no_loops, pal)
    assert r.n_vertices == int(re.search(r"unitig graph size: (\d+)", log).group(1))
    assert r.n_loops == int(re.search(r"number looped: (\d+)", log).group(1))
    assert r.n_standalone == int(re.search(r"number isolated: (\d+)", log).group(1))
    v, text = engine.unitig_contigs()
    assert v.size == r.n_vertices and sum(map(len, text)) == r.n_bases
    assert all(len(t) == k + n for t, n in zip(text, v["length"]))
