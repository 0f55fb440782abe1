"""Writes tests/golden/unitig_clean.json: for a few synthetic libraries, what the reference's own
`megahit_core assemble -t 1 --bubble_level 0 --prune_level 0 --cleaning_rounds N` (N >= 1) does on the SdBG of its own
`read2sdbg` — the digests of the six output files and, parsed from its log, the per-round "Number unitigs disconnected" and
"Tips removed" counts, the initial "unitig graph size" and the final "number contigs / isolated / looped".
tests/test_gpu_unitig_clean_golden.py compares mhx_core (MHX_ASSEMBLE_CLEAN=1) against them without the reference.  Runs on
the CPU:

    python tools/make_unitig_clean_golden.py [--ref oracle/_ref/ref_megahit_core]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_unitig_golden as mug  # noqa: E402
from megahit_amd import synth  # noqa: E402

QUAL = ["--bubble_level", "0", "--prune_level", "0"]
FILES = mug.FILES
A = dict(kind="linear", G=20000, pairs=4000, err=0.01, seed=31, read_len=100, frag=250, k=21, m=2, mercy=False)
B = dict(kind="linear", G=20000, pairs=4000, err=0.02, seed=41, read_len=100, frag=250, k=21, m=1, mercy=False)
C = dict(kind="circular", G=8000, pairs=3000, err=0.01, seed=43, read_len=100, frag=250, k=29, m=2, mercy=False)
D = dict(kind="palindrome", G=6000, pairs=3000, err=0.01, seed=44, read_len=100, frag=250, k=25, m=2, mercy=False)
E = dict(kind="linear", G=20000, pairs=4000, err=0.01, seed=45, read_len=150, frag=300, k=63, m=2, mercy=True)
CASES = [  # name, library + graph, cleaning rounds, further assemble options
    dict(A, name="A", rounds=5, opts=[]),
    dict(B, name="B", rounds=5, opts=[]),
    dict(C, name="C", rounds=5, opts=[]),
    dict(D, name="D", rounds=5, opts=[]),
    dict(E, name="E", rounds=5, opts=[]),
    dict(A, name="A-1round", rounds=1, opts=[]),
    dict(B, name="B-1round", rounds=1, opts=[]),
    # A's shape with another seed: with seed 31 no tip is left below 10 after the SdBG-level trimming
    dict(A, seed=47, name="A-tip10-standalone", rounds=5, opts=["--max_tip_len", "10", "--output_standalone", "--min_standalone", "0"]),
    dict(A, name="A-tip0", rounds=5, opts=["--max_tip_len", "0"]),
    dict(B, name="B-ratio0.3", rounds=5, opts=["--disconnect_ratio", "0.3"]),
    # A plus a 30-base circle: a loop vertex shorter than the tip thresholds, deleted by RemoveTips in round 2 (its edges stay
    # valid: Refresh does not invalidate a deleted loop, and the finish must leave that cycle out)
    dict(A, kind="linear+plasmid", plasmid=30, name="A-plasmid", rounds=5, opts=[]),
    # S + revcomp(S) closed to a circle: after cleaning the whole graph is one cycle that is its own reverse complement
    dict(kind="selfrc-circular", G=3000, pairs=3000, err=0.01, seed=51, read_len=100, frag=250, k=25, m=2, mercy=False, name="selfrc-circle",
         rounds=5, opts=[]),
]


def write_library(d, c):
    """make_unitig_golden.write_library plus two kinds of its own; deterministic in c"""
    import numpy as np
    if c["kind"] == "linear+plasmid":
        g = np.random.default_rng(c["seed"]).integers(0, 4, size=c["G"], dtype=np.uint8)
        reads = synth.gen_pe_reads(c["pairs"], g.size, read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"] + 1, genome=g)
        ring = np.tile(np.random.default_rng(c["seed"] + 2).integers(0, 4, size=c["plasmid"], dtype=np.uint8), 20)  # the circle, unrolled
        extra = synth.gen_pe_reads(200, ring.size, read_len=c["read_len"], frag=c["frag"], err=0.0, seed=c["seed"] + 3, genome=ring)
        reads = np.concatenate([reads, extra])
    elif c["kind"] == "selfrc-circular":
        s = np.random.default_rng(c["seed"]).integers(0, 4, size=c["G"], dtype=np.uint8)
        g = np.concatenate([s, (3 - s)[::-1]])
        g = np.concatenate([g, g[:c["frag"] + c["read_len"]]])
        reads = synth.gen_pe_reads(c["pairs"], g.size, read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"] + 1, genome=g)
    else:
        return mug.write_library(d, c)
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [reads])
    return prefix


def assemble_args(c):
    return QUAL + ["--cleaning_rounds", str(c["rounds"])] + c["opts"]


def parse_log(text):
    """the counts a cleaning run logs (the reference's lines, which mhx_core prints alike)"""
    stat = re.findall(r"number contigs: (\d+), number isolated: (\d+), number looped: (\d+)", text)
    return dict(
        graph_size=int(re.search(r"unitig graph size: (\d+)", text).group(1)),
        disconnected=[int(x) for x in re.findall(r"Number unitigs disconnected: (\d+)", text)],
        tips=[int(x) for x in re.findall(r"Tips removed: (\d+)", text)],
        rounds_run=len(re.findall(r"Graph cleaning round \d+", text)),
        final=dict(zip(("contigs", "isolated", "looped"), (int(x) for x in stat[-1]))),
        looped_before=int(stat[0][2]),
    )


def run_reference(ref, c, d, threads=1):
    """reads -> the reference's read2sdbg -> its assemble; returns (output prefix, log)"""
    lib = write_library(d, c)
    g = os.path.join(d, "g")
    subprocess.run([ref, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", lib, "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = os.path.join(d, "ref")
    p = subprocess.run([ref, "assemble", "-s", g, "-o", out, "-t", str(threads)] + assemble_args(c), check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    return out, p.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    a = ap.parse_args()
    cases = []
    for c in CASES:
        with tempfile.TemporaryDirectory() as d:
            out, log = run_reference(a.ref, c, d)
            rec = dict(c, digests=mug.digests(out), log=parse_log(log))
        # a case that cleans nothing shows nothing: change its seed instead of keeping it
        assert rec["log"]["disconnected"][0] > 0, (c["name"], rec["log"])
        if c["rounds"] > 1 and c["opts"][:2] != ["--max_tip_len", "0"]:
            assert sum(rec["log"]["tips"]) > 0, (c["name"], rec["log"])
        if c["name"] == "A-plasmid":  # the loop is there before cleaning and gone after
            assert rec["log"]["looped_before"] == 1 and rec["log"]["final"]["looped"] == 0, rec["log"]
        cases.append(rec)
        print(c["name"], rec["log"], file=sys.stderr)
    with open(os.path.join(ROOT, "tests", "golden", "unitig_clean.json"), "w") as f:
        json.dump({"what": "reference megahit_core assemble -t 1 " + " ".join(QUAL) + " --cleaning_rounds N on its own read2sdbg graph", "cases": cases},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
