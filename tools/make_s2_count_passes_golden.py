"""Generate tests/golden/s2_count_passes.json: the digests of the REFERENCE's own `read2sdbg` (-k 27 -m 1, -k 25 -m 2) on the
200 000-read library of tests/test_gpu_memory_plan.py, for tests/test_gpu_s2_count_passes_cli.py.

Runs oracle/_ref/ref_megahit_core (the reference's sources compiled in place by oracle/Makefile) on the CPU and records the
canonical-stream digests of its outputs (megahit_amd/canon.py) and the md5 of the library's record stream: digests only.

    python tools/make_s2_count_passes_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megahit_amd import canon, synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core")
PATH = os.path.join(ROOT, "tests", "golden", "s2_count_passes.json")
# the "fixed" library of tests/test_gpu_memory_plan.py (its `libs` fixture): a random genome, read pairs of 100 bases with errors
LIBRARY = dict(genome=2000000, genome_seed=41, pairs=100000, read_len=100, frag=250, err=0.005, seed=42)
CASES = [(27, 1), (25, 2)]


def write_library(prefix):
    genome = np.random.default_rng(LIBRARY["genome_seed"]).integers(0, 4, size=LIBRARY["genome"], dtype=np.uint8)
    reads = synth.gen_pe_reads(LIBRARY["pairs"], LIBRARY["genome"], read_len=LIBRARY["read_len"], frag=LIBRARY["frag"], err=LIBRARY["err"], seed=LIBRARY["seed"],
                               genome=genome)
    return synth.write_read_lib(prefix, [reads])


def main():
    tmp = tempfile.mkdtemp(prefix="mhx_s2cp_")
    prefix = os.path.join(tmp, "fixed")
    n_reads, n_bases = write_library(prefix)
    gold = {"library": dict(LIBRARY, reads=int(n_reads), bases=int(n_bases), bin_md5=canon.digest_file(prefix + ".bin")), "cases": []}
    for k, m in CASES:
        out = os.path.join(tmp, "ref_k%d_m%d" % (k, m))
        subprocess.run([REF, "read2sdbg", "-k", str(k), "-m", str(m), "--read_lib_file", prefix, "--output_prefix", out, "--host_mem", "2e9", "--num_cpu_threads", "3"],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        ent = {"k": k, "m": m, "sdbg": canon.digest_sdbg(out)}
        if os.path.exists(out + ".counting"):
            ent["counting"] = canon.digest_file(out + ".counting")
        gold["cases"].append(ent)
    with open(PATH, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % PATH)


if __name__ == "__main__":
    main()
