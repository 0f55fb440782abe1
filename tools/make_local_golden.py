#!/usr/bin/env python3
"""Writes tests/golden/local_map.json: for every case of tests/local_cases.py the numbers the reference's `local` logs
(oracle/_ref/ref_megahit_core local -t 1) on the case's files, which are made from the case's seed here and again by the
tests.  Only seeds, options and those numbers are stored.

Checks while generating that the cases have teeth: some library with aligned < total, some paired library whose range is not
max_read_len - 1, some index smaller than its number of seed slots, some added > 0.  The reference's log does not tell the two
contig ends apart: that items exist at the start and at the end of a contig is asserted in tests/test_local_model_golden.py,
on the model's items of the cases whose counts equal the reference's.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_cases  # noqa: E402
import local_model  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core")
DEFAULT = dict(seed_kmer=31, sparsity=8, min_mapping_len=75, similarity=0.8)
CASES = [
    dict(name="pe150", seed=11),
    dict(name="lengths", seed=12),
    dict(name="noisy_single", seed=13),
    dict(name="overhang", seed=14),
    dict(name="overhang", seed=14, sparsity=1),
    dict(name="repeat", seed=15),
    dict(name="rc_ends", seed=16),
    dict(name="rc_ends", seed=16, sparsity=1),
    dict(name="two_libs", seed=17, seed_kmer=24, sparsity=1),
    dict(name="two_libs", seed=17, seed_kmer=24),
    dict(name="no_contig", seed=18),
    dict(name="seed32", seed=20, seed_kmer=32, sparsity=1),
    dict(name="seed32", seed=20, seed_kmer=32),
    dict(name="seed32_dup", seed=20, seed_kmer=32),
    dict(name="two_batches", seed=19),
]


def parse_log(text):
    """the numbers of the reference's log lines of the first half -> dict"""
    out = {"libs": {}}
    m = re.search(r"Number of contigs: (\d+), index size: (\d+)", text)
    out["n_contigs"], out["index_size"] = int(m.group(1)), int(m.group(2))
    for m in re.finditer(r"Lib (\d+), insert size: (\S+) sd: (\S+)", text):
        out["libs"].setdefault(int(m.group(1)), {}).update(mean=m.group(2), sd=m.group(3))
    for m in re.finditer(r"Lib (\d+): total (\d+) reads, aligned (\d+), added (\d+) reads to local assembly", text):
        out["libs"].setdefault(int(m.group(1)), {}).update(total=int(m.group(2)), aligned=int(m.group(3)), added=int(m.group(4)))
    m = re.search(r"Minimum number of reads to do local assembly: (\d+)", text)
    out["min_reads"] = int(m.group(1))
    out["libs"] = [out["libs"][i] for i in sorted(out["libs"])]
    return out


def run_reference(case, threads=1):
    with tempfile.TemporaryDirectory() as d:
        fa, prefix = local_cases.write_files(case, d)
        cmd = [REF, "local", "-c", fa, "-l", prefix, "-o", os.path.join(d, "out.fa"), "-t", str(threads), "--seed_kmer", str(case["seed_kmer"]),
               "--sparsity", str(case["sparsity"]), "--min_mapping_len", str(case["min_mapping_len"]), "--similarity", repr(case["similarity"]),
               "--min_contig_len", str(local_cases.MIN_CONTIG_LEN)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        if p.returncode != 0:
            raise SystemExit("%s failed:\n%s" % (" ".join(cmd), p.stdout))
        return parse_log(p.stdout)


def main():
    out = []
    teeth = dict(unaligned=False, range=False, dup=False, added=False)
    for spec in CASES:
        case = dict(DEFAULT, **spec)
        case["ref"] = ref = run_reference(case)
        contigs, libs = local_cases.build(case)
        kept = local_model.keep_contigs(contigs, local_cases.MIN_CONTIG_LEN)
        slots = sum((len(c) - case["seed_kmer"] + case["sparsity"]) // case["sparsity"] for c in kept if len(c) >= case["seed_kmer"])
        case["seed_slots"] = slots
        for (b, e, mx, paired), lib in zip(local_cases.lib_table(libs), ref["libs"]):
            teeth["unaligned"] |= lib["aligned"] < lib["total"]
            teeth["added"] |= lib["added"] > 0
            if paired:
                mean, sd = float(lib["mean"]), float(lib["sd"])
                rng = mx - 1 if mean < mx else int(min(2 * mean, mean + 3 * sd))
                teeth["range"] |= min(rng, 650) != mx - 1
        teeth["dup"] |= ref["index_size"] < slots
        print(json.dumps(case))
        out.append(case)
    missing = [k for k, v in teeth.items() if not v]
    if missing:
        raise SystemExit("the cases have no teeth for: %s (choose other seeds)" % ", ".join(missing))
    path = os.path.join(ROOT, "tests", "golden", "local_map.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
