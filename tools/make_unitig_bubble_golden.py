"""Writes tests/golden/unitig_bubble.json: for a few synthetic libraries, what the reference's own
`megahit_core assemble -t 1 --bubble_level 1|2 --prune_level 0|2|3 [--careful_bubble]` does on the SdBG of its own `read2sdbg` —
the digests of the eight output files (make_unitig_prune_golden.FILES) and, parsed from its log, the counts of
make_unitig_clean_golden.parse_log plus, per round, "Number of bubbles removed", "Number of complex bubbles removed" and
"Unitigs removed in (more-)excessive pruning" / "in excessive pruning", the final "local low depth unitigs removed / complex
bubbles removed" pair and the number of .bubble_seq.fa and .addi.fa records.  tests/test_gpu_unitig_bubble_golden.py compares
mhx_core (MHX_ASSEMBLE_BUBBLE=1) against them without the reference.  Runs on the CPU:

    python tools/make_unitig_bubble_golden.py [--ref oracle/_ref/ref_megahit_core]

Library kind "diploid": a genome g and a second haplotype h = g with a variant every `gap` bases, cycling through an SNP, two
SNPs `near` bases apart, a deletion of 1-3 bases and an insertion of 1-3 bases; `pairs` read pairs from g and minor * pairs
from h.  An SNP is a bubble of k + 1 edges (the naive remover's), the other three are longer or of unequal arms (the complex
remover's)."""
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
import make_unitig_prune_golden as mpg  # noqa: E402
from megahit_amd import synth  # noqa: E402

mcg = mpg.mcg
FILES = mpg.FILES
A = dict(kind="diploid", G=20000, pairs=4000, err=0.01, seed=61, read_len=100, frag=250, k=21, m=2, mercy=False, gap=150, near=8, minor=0.5)
B = dict(kind="diploid", G=20000, pairs=4000, err=0.01, seed=62, read_len=150, frag=300, k=63, m=2, mercy=False, gap=300, near=20, minor=0.7)
C = dict(kind="diploid", G=60000, pairs=12000, err=0.02, seed=71, read_len=100, frag=250, k=21, m=1, mercy=False, gap=200, near=8, minor=0.5)
ORCH = ["--merge_len", "20", "--merge_similar", "0.95"]  # what the orchestrator passes
CASES = [  # name, library + graph, bubble level, prune level, final round, careful, minimum depth, cleaning rounds, further options
    dict(A, name="A-b1", bubble=1, prune=2, final=False, careful=False, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b2", bubble=2, prune=2, final=False, careful=False, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b2-careful", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b2-careful-final", bubble=2, prune=2, final=True, careful=True, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b1-careful-p0", bubble=1, prune=0, final=False, careful=True, min_depth=2, rounds=5, opts=ORCH),
    # assemble's own defaults, --merge_len 20 --merge_similar 0.98: the bubbles that pop at 0.95 are candidates here too (0.98 only
    # narrows the length test), and their strings of 43 to ~60 characters have max_indel = (int)(len * 0.02) <= 1: the similarity fails
    dict(A, name="A-b2-p0-sim0.98", bubble=2, prune=0, final=False, careful=False, min_depth=2, rounds=5, opts=[]),
    dict(A, name="A-b2-p3-careful", bubble=2, prune=3, final=False, careful=True, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b1-p3-final", bubble=1, prune=3, final=True, careful=False, min_depth=2, rounds=5, opts=ORCH),
    dict(A, name="A-b2-merge0", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=["--merge_len", "0", "--merge_similar", "0.95"]),
    # max_len = lround(1 * 21 / 0.99) = 21 and 21 * 0.01 < 1: the complex pass returns before it looks at the graph
    dict(A, name="A-b2-early-return", bubble=2, prune=2, final=False, careful=False, min_depth=2, rounds=5,
         opts=["--merge_len", "1", "--merge_similar", "0.99"]),
    dict(A, name="A-b2-rounds1", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=1, opts=ORCH),
    dict(B, name="B-b2-careful", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=ORCH),
    dict(B, name="B-b2-final", bubble=2, prune=2, final=True, careful=False, min_depth=2, rounds=5, opts=ORCH),
    dict(C, name="C-b2-m1", bubble=2, prune=2, final=False, careful=True, min_depth=2, rounds=5, opts=ORCH),
    dict(C, name="C-b2-m1-p3", bubble=2, prune=3, final=False, careful=False, min_depth=2, rounds=5, opts=ORCH),
    # the special graphs of the cleaning golden (S + revcomp(S); the same closed to a circle) with a second haplotype
    dict(mcg.D, kind="diploid-palindrome", gap=150, near=8, minor=0.5, name="D-palindrome-b2", bubble=2, prune=2, final=False, careful=True,
         min_depth=2, rounds=5, opts=ORCH),
    dict(mpg.SELFRC, kind="diploid-selfrc-circular", gap=150, near=8, minor=0.5, name="selfrc-circle-b2", bubble=2, prune=2, final=False,
         careful=True, min_depth=2, rounds=5, opts=ORCH),
]
LIBRARY = ("kind", "G", "pairs", "err", "seed", "read_len", "frag", "k", "m", "mercy", "gap", "near", "minor")


def second_haplotype(g, c):
    """g with a variant every c['gap'] bases: SNP, two SNPs c['near'] apart, deletion, insertion, and round again"""
    import numpy as np
    rng = np.random.default_rng(c["seed"] + 7)
    parts, last = [], 0
    for i, pos in enumerate(range(c["gap"], g.size - c["gap"], c["gap"])):
        kind = i % 4
        n = int(rng.integers(1, 4))
        if kind in (0, 1):
            seg = g[last:pos + 1].copy()
            seg[-1] = (seg[-1] + int(rng.integers(1, 4))) % 4
            if kind == 1:
                seg[-1 - c["near"]] = (seg[-1 - c["near"]] + int(rng.integers(1, 4))) % 4
            parts.append(seg)
            last = pos + 1
        elif kind == 2:
            parts.append(g[last:pos])
            last = pos + n
        else:
            parts.append(g[last:pos])
            parts.append(rng.integers(0, 4, size=n, dtype=np.uint8))
            last = pos
    parts.append(g[last:])
    return np.concatenate(parts).astype(np.uint8)


def write_library(d, c):
    """make_unitig_clean_golden.write_library plus the diploid kinds; deterministic in c"""
    import numpy as np
    if not c["kind"].startswith("diploid"):
        return mcg.write_library(d, c)
    s = np.random.default_rng(c["seed"]).integers(0, 4, size=c["G"], dtype=np.uint8)
    hs = second_haplotype(s, c)

    def shape(x):
        if c["kind"] == "diploid":
            return x
        x = np.concatenate([x, (3 - x)[::-1]])  # its own reverse complement
        if c["kind"] == "diploid-selfrc-circular":
            x = np.concatenate([x, x[:c["frag"] + c["read_len"]]])
        return x

    g, h = shape(s), shape(hs)
    reads = [synth.gen_pe_reads(c["pairs"], g.size, read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"] + 1, genome=g),
             synth.gen_pe_reads(int(c["pairs"] * c["minor"]), h.size, read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"] + 2, genome=h)]
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [np.concatenate(reads)])
    return prefix


def assemble_args(c):
    return ["--bubble_level", str(c["bubble"]), "--prune_level", str(c["prune"]), "--min_depth", str(c["min_depth"]), "--cleaning_rounds",
            str(c["rounds"])] + (["--is_final_round"] if c["final"] else []) + (["--careful_bubble"] if c["careful"] else []) + c["opts"]


def parse_log(text):
    """make_unitig_clean_golden.parse_log plus the bubble and pruning counts (the reference's lines, which mhx_core prints alike)"""
    out = mcg.parse_log(text)
    out["naive"] = [int(x) for x in re.findall(r"Number of bubbles removed: (\d+)", text)]
    out["complex"] = [int(x) for x in re.findall(r"Number of complex bubbles removed: (\d+)", text)]
    out["pruned"] = [int(x) for x in re.findall(r"Unitigs removed in excessive pruning: (\d+)", text)]
    out["more_pruned"] = [int(x) for x in re.findall(r"Unitigs removed in \(more-\)excessive pruning: (\d+)", text)]
    m = re.search(r"Number of local low depth unitigs removed: (\d+), complex bubbles removed: (\d+)", text)
    out["final_pass"] = [int(m.group(1)), int(m.group(2))] if m else None
    return out


def records(path):
    with open(path, "rb") as f:
        return f.read().count(b">")


def build_graph(ref, c, d):
    """reads -> the reference's read2sdbg; returns the graph's prefix"""
    lib = write_library(d, c)
    g = os.path.join(d, "g")
    subprocess.run([ref, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", lib, "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return g


def reference_answer(ref, g, out, c, threads=1):
    """the reference's assemble on graph g -> (digests, counts)"""
    log = parse_log(mpg.run_assemble(ref, g, out, assemble_args(c), threads=threads))
    log["bubble_records"] = records(out + ".bubble_seq.fa")
    log["addi_records"] = records(out + ".addi.fa") if c["prune"] >= 1 else 0
    dig = mpg.digests(out)
    return dig, log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    a = ap.parse_args()
    cases, graphs = [], {}
    with tempfile.TemporaryDirectory() as top:
        for c in CASES:
            key = tuple(c.get(x) for x in LIBRARY)
            if key not in graphs:
                d = os.path.join(top, "g%d" % len(graphs))
                os.mkdir(d)
                graphs[key] = build_graph(a.ref, c, d)
            out = os.path.join(top, "ref-" + c["name"])
            dig, log = reference_answer(a.ref, graphs[key], out, c)
            # a case that pops nothing shows nothing: change its seed instead of keeping it
            assert sum(log["naive"]) > 0, (c["name"], log)
            early = c["name"] in ("A-b2-merge0", "A-b2-early-return", "A-b2-p0-sim0.98")
            if c["bubble"] >= 2:
                assert len(log["complex"]) == log["rounds_run"], (c["name"], log)
                assert (sum(log["complex"]) == 0) if early else (sum(log["complex"]) > 0), (c["name"], log)
            else:
                assert log["complex"] == [], (c["name"], log)
            assert (log["final_pass"] is None) == (c["prune"] == 0), (c["name"], log)
            assert len(log["more_pruned"]) == (log["rounds_run"] if c["prune"] == 3 else 0), (c["name"], log)
            if not c["careful"]:
                assert log["bubble_records"] == 0, (c["name"], log)
            cases.append(dict(c, digests=dig, log=log))
            print(c["name"], log, file=sys.stderr)
    assert any(c["log"]["final_pass"] and c["log"]["final_pass"][1] > 0 for c in cases)  # the final complex pop finds something
    assert any(c["careful"] and c["log"]["bubble_records"] > 0 for c in cases)
    assert any(c["careful"] and c["bubble"] == 1 and c["log"]["bubble_records"] > 0 for c in cases)
    assert any(c["prune"] == 3 and sum(c["log"]["more_pruned"]) > 0 for c in cases)
    assert any(c["final"] and sum(c["log"]["complex"]) > 0 for c in cases)
    # (a similarity check that passes: every complex count above; one that fails cannot be read off the reference's log —
    # tests/test_gpu_unitig_bubble_golden.py asserts it on the counters mhx_core logs)
    with open(os.path.join(ROOT, "tests", "golden", "unitig_bubble.json"), "w") as f:
        f.write('{"what": "reference megahit_core assemble -t 1 --bubble_level 1|2 --prune_level 0|2|3 [--careful_bubble] on its own read2sdbg graph",\n'
                ' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases) + "\n ]}\n")


if __name__ == "__main__":
    main()
