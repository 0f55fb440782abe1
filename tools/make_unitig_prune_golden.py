"""Writes tests/golden/unitig_prune.json: for a few synthetic libraries, what the reference's own
`megahit_core assemble -t 1 --bubble_level 0 --prune_level 1|2 --min_depth D` does on the SdBG of its own `read2sdbg` — the
digests of the eight output files (the six of make_unitig_golden.FILES plus .addi.fa and .addi.fa.info) and, parsed from its
log, the counts of make_unitig_clean_golden.parse_log plus the per-round "Unitigs removed in excessive pruning", the "Number
of local low depth unitigs removed" and the number of .addi.fa records.  tests/test_gpu_unitig_prune_golden.py compares
mhx_core (MHX_ASSEMBLE_PRUNE=1) against them without the reference.  Runs on the CPU:

    python tools/make_unitig_prune_golden.py [--ref oracle/_ref/ref_megahit_core]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_unitig_clean_golden as mcg  # noqa: E402
import make_unitig_golden as mug  # noqa: E402

FILES = mug.FILES + [".addi.fa", ".addi.fa.info"]
SELFRC = dict(kind="selfrc-circular", G=3000, pairs=3000, err=0.01, seed=51, read_len=100, frag=250, k=25, m=2, mercy=False)
CASES = [  # name, library + graph, prune level, final round, minimum depth, cleaning rounds, further assemble options
    dict(mcg.A, name="A-p2", prune=2, final=False, min_depth=2, rounds=5, opts=[]),
    dict(mcg.A, name="A-p2-final", prune=2, final=True, min_depth=2, rounds=5, opts=[]),
    dict(mcg.A, name="A-p1", prune=1, final=False, min_depth=2, rounds=5, opts=[]),
    dict(mcg.A, name="A-p1-final", prune=1, final=True, min_depth=2, rounds=5, opts=[]),
    dict(mcg.A, name="A-rounds0-p1", prune=1, final=False, min_depth=2, rounds=0, opts=[]),
    dict(mcg.A, name="A-standalone-final", prune=2, final=True, min_depth=2, rounds=5, opts=["--output_standalone", "--min_standalone", "0"]),
    # min(low_local_ratio, 0.1) = 0.05 inside the rounds.  DisconnectWeakLinks at its default ratio of 0.1 isolates nearly every
    # vertex that 0.05 of the local mean could catch before the pruning sees it, so this case disconnects at 0.02 (m = 1, 6000 pairs)
    dict(mcg.B, err=0.01, pairs=6000, name="B-ratio0.05", prune=2, final=False, min_depth=4, rounds=5,
         opts=["--low_local_ratio", "0.05", "--disconnect_ratio", "0.02"]),
    # m = 1: edges seen once are in the graph, so a minimum depth of 2 removes vertices inside the rounds
    dict(mcg.B, name="B-m1", prune=2, final=False, min_depth=2, rounds=5, opts=[]),
    dict(mcg.B, name="B-m1-final", prune=2, final=True, min_depth=2, rounds=5, opts=[]),
    # the special graphs of the cleaning golden, at about half its coverage and twice its error rate: at 75 x and 1 % errors the
    # rounds leave one clean contig and the pruning finds nothing to remove
    dict(mcg.C, pairs=1500, err=0.02, name="C-circular", prune=2, final=False, min_depth=2, rounds=5, opts=[]),  # the merged cycle is changed
    dict(mcg.D, pairs=1500, err=0.02, name="D-palindrome", prune=2, final=False, min_depth=3, rounds=5, opts=[]),
    dict(mcg.E, name="E-k63-final", prune=2, final=True, min_depth=2, rounds=5, opts=[]),
    dict(mcg.A, kind="linear+plasmid", plasmid=30, name="A-plasmid", prune=2, final=False, min_depth=2, rounds=5, opts=[]),
    dict(SELFRC, pairs=800, err=0.03, name="selfrc-circle", prune=2, final=False, min_depth=2, rounds=5, opts=[]),
    # the same with another seed: the iteration's Refresh closes the self-complementary cycle, whose survivor deletes itself
    dict(SELFRC, pairs=800, err=0.03, seed=53, name="selfrc-circle-vanishes", prune=2, final=False, min_depth=2, rounds=5, opts=[]),
]


def assemble_args(c):
    return ["--bubble_level", "0", "--prune_level", str(c["prune"]), "--min_depth", str(c["min_depth"]), "--cleaning_rounds", str(c["rounds"])] + \
        (["--is_final_round"] if c["final"] else []) + c["opts"]


def parse_log(text):
    """make_unitig_clean_golden.parse_log plus the pruning counts (the reference's lines, which mhx_core prints alike)"""
    out = mcg.parse_log(text)
    out["pruned"] = [int(x) for x in re.findall(r"Unitigs removed in excessive pruning: (\d+)", text)]
    out["low_depth_removed"] = int(re.search(r"Number of local low depth unitigs removed: (\d+), complex bubbles removed: 0", text).group(1))
    return out


def digests(prefix):
    out = {}
    for s in FILES:
        if os.path.exists(prefix + s):  # (a final round writes no .addi.fa records but the file is there: prune level >= 1)
            with open(prefix + s, "rb") as f:
                out[s] = hashlib.sha256(f.read()).hexdigest()
    return out


def addi_records(prefix):
    with open(prefix + ".addi.fa", "rb") as f:
        return f.read().count(b">")


def build_graph(ref, c, d):
    """reads -> the reference's read2sdbg; returns the graph's prefix"""
    lib = mcg.write_library(d, c)
    g = os.path.join(d, "g")
    subprocess.run([ref, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", lib, "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return g


def run_assemble(ref, g, out, args, threads=1):
    p = subprocess.run([ref, "assemble", "-s", g, "-o", out, "-t", str(threads)] + args, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    return p.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    a = ap.parse_args()
    cases = []
    for c in CASES:
        with tempfile.TemporaryDirectory() as d:
            g = build_graph(a.ref, c, d)
            out = os.path.join(d, "ref")
            log = parse_log(run_assemble(a.ref, g, out, assemble_args(c)))
            log["addi_records"] = addi_records(out)
            rec = dict(c, digests=digests(out), log=log)
            # the same graph and options at prune level 0: what the pruning changed
            base = os.path.join(d, "base")
            run_assemble(a.ref, g, base, assemble_args(dict(c, prune=0)))
            rec["contigs_differ_from_prune0"] = mug.digests(base)[".contigs.fa"] != rec["digests"][".contigs.fa"]
        assert sorted(rec["digests"]) == sorted(FILES), (c["name"], sorted(rec["digests"]))
        # a case that prunes nothing shows nothing: change its seed instead of keeping it
        assert log["low_depth_removed"] > 0, (c["name"], log)
        if c["prune"] >= 2 and c["rounds"] > 0:
            assert len(log["pruned"]) == log["rounds_run"], (c["name"], log)
        else:
            assert log["pruned"] == [], (c["name"], log)
        if c["name"].startswith("B-m1") or c["name"] == "B-ratio0.05":
            assert sum(log["pruned"]) > 0, (c["name"], log)
        if c["final"]:
            assert log["addi_records"] == 0, (c["name"], log)
        cases.append(rec)
        print(c["name"], log, rec["contigs_differ_from_prune0"], file=sys.stderr)
    assert any(c["prune"] == 2 and sum(c["log"]["pruned"]) > 0 for c in cases)
    assert any(not c["final"] and c["log"]["addi_records"] > 0 for c in cases)
    assert any(c["final"] and c["contigs_differ_from_prune0"] for c in cases)
    with open(os.path.join(ROOT, "tests", "golden", "unitig_prune.json"), "w") as f:
        # one case per line: the digests are most of the file
        f.write('{"what": "reference megahit_core assemble -t 1 --bubble_level 0 --prune_level 1|2 --min_depth D on its own read2sdbg graph",\n'
                ' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases) + "\n ]}\n")


if __name__ == "__main__":
    main()
