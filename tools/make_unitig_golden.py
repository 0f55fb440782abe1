"""Writes tests/golden/unitigs.json: for a few synthetic libraries, the digests of what the reference's own
`megahit_core assemble -t 1 --bubble_level 0 --prune_level 0 --cleaning_rounds 0` writes on the SdBG of its own
`read2sdbg` (.contigs.fa, .final.contigs.fa, .bubble_seq.fa and their .info files).  tests/test_gpu_unitigs_golden.py
compares mhx_core against them without the reference.  Runs on the CPU:

    python tools/make_unitig_golden.py [--ref oracle/_ref/ref_megahit_core]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megahit_amd import synth  # noqa: E402

QUAL = ["--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"]
FILES = [".contigs.fa", ".contigs.fa.info", ".final.contigs.fa", ".final.contigs.fa.info", ".bubble_seq.fa", ".bubble_seq.fa.info"]
CASES = [  # library (synthetic, see write_library), graph (k, m, mercy), assemble options
    dict(kind="linear", G=20000, pairs=4000, err=0.01, seed=31, read_len=100, frag=250, k=21, m=2, mercy=False, opts=[]),
    dict(kind="linear", G=20000, pairs=4000, err=0.01, seed=32, read_len=150, frag=300, k=63, m=2, mercy=True,
         opts=["--output_standalone", "--min_standalone", "200"]),
    dict(kind="circular", G=8000, pairs=3000, err=0.002, seed=33, read_len=100, frag=250, k=29, m=2, mercy=False, opts=["--max_tip_len", "10"]),
    dict(kind="palindrome", G=6000, pairs=3000, err=0.0, seed=34, read_len=100, frag=250, k=21, m=2, mercy=False,
         opts=["--output_standalone", "--min_standalone", "0"]),
]


def write_library(d, c):
    """reads of a linear / circular / S + revcomp(S) genome -> <d>/reads.{bin,lib_info}; deterministic in c"""
    import numpy as np
    g = np.random.default_rng(c["seed"]).integers(0, 4, size=c["G"], dtype=np.uint8)
    if c["kind"] == "palindrome":
        g = np.concatenate([g, (3 - g)[::-1]])
    elif c["kind"] == "circular":
        g = np.concatenate([g, g[:c["frag"] + c["read_len"]]])
    reads = synth.gen_pe_reads(c["pairs"], g.size, read_len=c["read_len"], frag=c["frag"], err=c["err"], seed=c["seed"] + 1, genome=g)
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [reads])
    return prefix


def digests(prefix):
    out = {}
    for s in FILES:
        with open(prefix + s, "rb") as f:
            out[s] = hashlib.sha256(f.read()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    a = ap.parse_args()
    cases = []
    for c in CASES:
        with tempfile.TemporaryDirectory() as d:
            lib = write_library(d, c)
            g = os.path.join(d, "g")
            subprocess.run([a.ref, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                            "--read_lib_file", lib, "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []), check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            out = os.path.join(d, "ref")
            subprocess.run([a.ref, "assemble", "-s", g, "-o", out, "-t", "1"] + QUAL + c["opts"], check=True, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            cases.append(dict(c, digests=digests(out)))
            print(c["kind"], c["k"], cases[-1]["digests"][".contigs.fa.info"], file=sys.stderr)
    with open(os.path.join(ROOT, "tests", "golden", "unitigs.json"), "w") as f:
        json.dump({"what": "reference megahit_core assemble -t 1 " + " ".join(QUAL) + " on its own read2sdbg graph", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
