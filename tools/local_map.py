#!/usr/bin/env python3
"""The first half of `megahit_core local` through the C ABI (mhx_local_index / _map / _insert_size / _collect): prints the
log lines the reference prints for it,

    Number of contigs: N, index size: M
    Lib i, insert size: MEAN sd: SD                      (paired libraries)
    Lib i: total T reads, aligned A, added D reads to local assembly
    Minimum number of reads to do local assembly: R

from a contigs FASTA (as `assemble` writes it) and a read library prefix (<prefix>.lib_info + <prefix>.bin).

    python tools/local_map.py -c contigs.fa -l reads [--seed_kmer 31 --sparsity 8 --min_mapping_len 75 --similarity 0.8 --min_contig_len 200]
        [--bench [--runs 5] [--ref oracle/_ref/ref_megahit_core] [--ref-threads 16] [--ref-timeout 900]]

--bench: one JSON line more: the wall times of index / map / insert size / collect (every run and the median), and the
reference's own timers ("Hash mapper construction", "Insert size estimation", "Mapping", "Local assembly" time elapsed) from one
run of `<ref> local -t <threads>` on the same files, with whether its log lines equal ours.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megahit_amd import lib, synth  # noqa: E402

LOOP_FLAG = 2
LINE_PATTERNS = (r"Number of contigs: \d+, index size: \d+", r"Lib \d+, insert size: \S+ sd: \S+",
                 r"Lib \d+: total \d+ reads, aligned \d+, added \d+ reads to local assembly",
                 r"Minimum number of reads to do local assembly: \d+")


def read_lib_info(prefix):
    """-> [(begin, end, max length, paired)] of <prefix>.lib_info (a line of totals, then two lines per library)"""
    with open(prefix + ".lib_info") as f:
        lines = f.read().split("\n")
    libs = []
    for i in range(2, len(lines), 2):
        if lines[i].strip():
            b, e, m, p = lines[i].split()[:4]
            libs.append((int(b), int(e), int(m), bool(int(p))))
    return libs


def read_library(prefix):
    """-> (record words, read lengths uint32 [n], library table)"""
    libs = read_lib_info(prefix)
    rec = np.fromfile(prefix + ".bin", dtype=np.uint32)
    n = libs[-1][1] if libs else 0
    if n and rec.size % n == 0 and rec.size // n == 1 + (int(rec[0]) + 15) // 16 and (rec[::rec.size // n] == rec[0]).all():
        lens = np.full(n, rec[0], dtype=np.uint32)  # reads of one length
    else:
        lens = np.empty(n, dtype=np.uint32)
        at = 0
        for i in range(n):
            lens[i] = rec[at]
            at += 1 + (int(rec[at]) + 15) // 16
    return rec, lens, libs


def read_contigs(path, min_len, discard_flags=LOOP_FLAG):
    """the contigs the reference's mapper keeps (long enough, not flagged), forward -> (packed words, start offsets, number)"""
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
        lut[ch + 32] = i
    kept, starts = [], [0]
    with open(path, "rb") as f:
        flag, seq = 0, []

        def flush():
            s = b"".join(seq)
            if s and len(s) >= min_len and not (flag & discard_flags):
                kept.append(lut[np.frombuffer(s, dtype=np.uint8)])
                starts.append(starts[-1] + len(s))

        first = True
        for line in f:
            if line.startswith(b">"):
                if not first:
                    flush()
                first = False
                m = re.search(rb"flag=(\d)", line)
                flag, seq = (int(m.group(1)) if m else 0), []
            else:
                seq.append(line.strip())
        if not first:
            flush()
    flat = np.concatenate(kept) if kept else np.zeros(0, dtype=np.uint8)
    words = synth.pack_reads_concat(flat[None, :]) if flat.size else np.zeros(0, dtype=np.uint32)
    return words, np.array(starts, dtype=np.uint64), len(kept)


def fmt(x):
    return "%.2f" % x


def run_once(e, a, words, start, n_ctg, libs, lens, times=None):
    """index + map + insert sizes + collect -> the log lines"""
    def clock(name, t0):
        if times is not None:
            times.setdefault(name, []).append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    n_keys = e.local_index(words, n_ctg, start, a.seed_kmer, a.sparsity)
    clock("index_s", t0)
    lines = ["Number of contigs: %d, index size: %d" % (n_ctg, n_keys)]
    t0 = time.perf_counter()
    e.local_map(a.min_mapping_len, a.similarity)
    clock("map_s", t0)
    t0 = time.perf_counter()
    rec = e.local_records()
    ranges = []
    for i, (b, en, mx, paired) in enumerate(libs):
        mean, sd, rng = lib.local_insert_size(rec, lens, b, en, mx, paired)
        ranges.append(rng)
        if paired:
            lines.append("Lib %d, insert size: %s sd: %s" % (i, fmt(mean), fmt(sd)))
    clock("insert_size_s", t0)
    t0 = time.perf_counter()
    aligned, added, items, offsets = e.local_collect([(b, en, p, r) for (b, en, mx, p), r in zip(libs, ranges)])
    clock("collect_s", t0)
    for i, (b, en, mx, paired) in enumerate(libs):
        lines.append("Lib %d: total %d reads, aligned %d, added %d reads to local assembly" % (i, en - b, aligned[i], added[i]))
    max_len = int(lens.max()) if lens.size else 0
    lines.append("Minimum number of reads to do local assembly: %d" % (max(ranges, default=0) // max_len if max_len else 1))
    return lines


def reference(a):
    """one run of the reference's `local` on the same files -> dict(timers, lines)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [a.ref, "local", "-c", a.contigs, "-l", a.lib, "-o", os.path.join(d, "out.fa"), "-t", str(a.ref_threads), "--seed_kmer", str(a.seed_kmer),
               "--sparsity", str(a.sparsity), "--min_mapping_len", str(a.min_mapping_len), "--similarity", repr(a.similarity), "--min_contig_len",
               str(a.min_contig_len)]
        out = {"threads": a.ref_threads}
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.ref_timeout)
            text = p.stdout
            out["returncode"] = p.returncode
        except subprocess.TimeoutExpired as ex:  # the mapping's lines come first: keep what was logged
            text = ex.stdout.decode() if isinstance(ex.stdout, bytes) else (ex.stdout or "")
            out["timed_out_after_s"] = a.ref_timeout
        out["wall_s"] = round(time.perf_counter() - t0, 3)
    for key, name in (("index_s", "Hash mapper construction"), ("read_lib_s", "Read lib"), ("insert_size_s", "Insert size estimation"),
                      ("map_s", "Mapping"), ("assemble_s", "Local assembly")):
        m = re.search(name + r" time elapsed: ([\d.]+)", text)
        out[key] = float(m.group(1)) if m else None
    out["lines"] = [m.group(0) for pat in LINE_PATTERNS for m in re.finditer(pat, text)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--contigs", required=True)
    ap.add_argument("-l", "--lib", required=True, help="read library prefix")
    ap.add_argument("--seed_kmer", type=int, default=31)
    ap.add_argument("--sparsity", type=int, default=8)
    ap.add_argument("--min_mapping_len", type=int, default=75)
    ap.add_argument("--similarity", type=float, default=0.8)
    ap.add_argument("--min_contig_len", type=int, default=200)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--ref-timeout", type=float, default=900)
    a = ap.parse_args()
    t0 = time.perf_counter()
    words, start, n_ctg = read_contigs(a.contigs, a.min_contig_len)
    rec, lens, libs = read_library(a.lib)
    t_read = time.perf_counter() - t0
    e = lib.Engine(0)
    t0 = time.perf_counter()
    e.load_bin_records(rec, lens.size, reverse=False)
    t_load = time.perf_counter() - t0
    lines = run_once(e, a, words, start, n_ctg, libs, lens)
    print("\n".join(lines))
    if a.bench:
        times = {}
        for _ in range(a.runs):
            assert run_once(e, a, words, start, n_ctg, libs, lens, times) == lines
        res = {"reads": int(lens.size), "contigs": n_ctg, "contig_bases": int(start[-1]), "host_read_files_s": round(t_read, 3),
               "load_reads_s": round(t_load, 3), "runs": {k: [round(x, 4) for x in v] for k, v in times.items()},
               "median": {k: round(statistics.median(v), 4) for k, v in times.items()}, "lines": lines}
        if os.path.exists(a.ref):
            ref = reference(a)
            # order as ours: contigs, insert sizes, totals, minimum; a NaN's sign is not compared
            res["ref"] = ref
            res["lines_equal"] = [l.replace("-nan", "nan") for l in ref["lines"]] == lines
            if ref.get("assemble_s") is not None and ref.get("map_s") is not None:
                first = (ref["index_s"] or 0) + (ref["insert_size_s"] or 0) + ref["map_s"]
                res["ref_first_half_share"] = round(first / (first + ref["assemble_s"]), 4)
        print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
