"""Structured small graphs through `mhx_core assemble` (MHX_ASSEMBLE_BUBBLE=1) against the reference's `assemble -t 1`, end to end.

    python tools/fuzz_assemble.py [SECONDS [SEED0]]   open-ended: cases SEED0, SEED0 + 1, ... until SECONDS are over (GPU + reference)
    python tools/fuzz_assemble.py --seed N            one case again; its directory is kept and printed
    python tools/fuzz_assemble.py --reference-only [SECONDS [SEED0]] | --reference-only --seed N
                                                      the reference alone (CPU): the counts per case, to choose the committed list
    python tools/fuzz_assemble.py --write-golden      tests/golden/assemble_fuzz.json for COMMITTED (the reference alone, CPU)

case(seed) draws, from the seed alone, a library and an option set.  The genome is a list of replicons (sequence, linear or circular,
coverage): a random backbone of 300..5000 bases that carries, at one place and 1..200 random bases apart, 0..6 planted motifs —
a tandem repeat of period 1..k+5, a forward copy and a reverse-complemented copy of a backbone segment of k-2..3k bases, a hairpin
x + revcomp(x) — and, as replicons of their own, rings of 2..4k bases, self-complementary rings x + revcomp(x) and (to reach the
unitig graph's tip removal, which random errors reach rarely) a stretch of the backbone that runs off into 1..3k bases of its own.
Half of the cases have a second haplotype of the main replicon: SNPs every 30..300 bases and 1..3 insertions or deletions of 1..3
bases.  Single-end reads of one length from both strands, circular replicons sampled across their origin, substitution errors.
Graph: k, m, mercy.  Assemble: every option `assemble_on_gpu()` of mhx_core.cpp serves with MHX_ASSEMBLE_BUBBLE=1.

Per case: the library, `mhx_core read2sdbg`, `mhx_core assemble` (MHX_ASSEMBLE_BUBBLE=1, MHX_REF_CORE a stub that fails) and
`ref_megahit_core assemble -t 1` on the same graph files with the same arguments; every output file byte for byte, which files
exist, and the logged counts.  Cases run one after another, every child process under its own time limit; the run stops at the
first non-zero exit, time limit or difference and starts nothing after it."""
import argparse
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_unitig_bubble_golden as mbg  # noqa: E402
from megahit_amd import canon, synth  # noqa: E402

mpg = mbg.mpg
FILES = mbg.FILES
REF = os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core")
MHX_CORE = os.path.join(ROOT, "megahit_amd", "mhx_core")
GOLDEN = os.path.join(ROOT, "tests", "golden", "assemble_fuzz.json")
GPU_TIMEOUT, REF_TIMEOUT = 120, 300

K_LIST = (17, 21, 25, 29, 31, 33, 47, 63, 79)
COVERAGES = (5, 8, 30, 60, 400)
ERRORS = (0.0, 0.0, 0.003, 0.01, 0.03)
MIN_DEPTHS = ("1", "1.5", "2", "3.7")
DISCONNECT = ("0", "0.05", "0.1", "0.3", "1.0")
LOW_LOCAL = ("0.05", "0.2", "0.5")
MERGE_LEN = (0, 1, 5, 20, 40, 60)
MERGE_SIMILAR = ("0.8", "0.9", "0.95", "0.98", "1.0")
MAX_K, SIM_MAX_LEN, SIM_MAX_INDEL = 255, 16384, 2047  # include/mhx.h: MHX_MAX_K, MHX_SIM_MAX_LEN, MHX_SIM_MAX_INDEL
# the committed list (tests/golden/assemble_fuzz.json): name -> seed.  Chosen with --reference-only so that the list as a whole
# meets the conditions tests/test_assemble_fuzz_golden.py asserts; a case cut down from a failure would stand here under a name
# that says what it is (none so far: no case has differed)
COMMITTED = [("seed-%d" % s, s) for s in (109, 129, 294, 309, 320, 348, 380, 389, 410, 434, 460, 461, 497, 533, 542, 573, 772, 782, 891, 920, 929, 1009, 1059, 1067, 1196, 1206, 1351, 1356, 1359, 1489, 1530, 1543)]


class ChildFailed(RuntimeError):
    """a child process left with a non-zero status"""
    def __init__(self, what, p):
        RuntimeError.__init__(self, "%s left with %d: %s" % (what, p.returncode, p.stderr[-1500:]))
        self.returncode = p.returncode


def tip_lens(k):
    """the --max_tip_len values at this k"""
    return (-1, 0, 1, 2, 10, k, 2 * k + 1, 500)


def fits_similarity_cap(merge_len, sim):
    """assemble_on_gpu()'s rule of mhx_core.cpp at k = MHX_MAX_K: the similarity kernel's cap (lround of a positive double)"""
    longest = float(math.floor(merge_len * MAX_K / sim + 0.5) + MAX_K)
    return longest <= SIM_MAX_LEN and longest * (1 - sim) < SIM_MAX_INDEL + 1


MERGE_PAIRS = [(ml, s) for ml in MERGE_LEN for s in MERGE_SIMILAR if fits_similarity_cap(ml, float(s))]


def revcomp(x):
    return (3 - x)[::-1]


def bases(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def second_haplotype(rng, g):
    """g with an SNP every `gap` bases and 1..3 insertions or deletions of 1..3 bases"""
    h = g.copy()
    gap = int(rng.integers(30, 301))
    for pos in range(gap, h.size - 1, gap):
        h[pos] = (h[pos] + int(rng.integers(1, 4))) % 4
    for _ in range(int(rng.integers(1, 4))):
        pos, n = int(rng.integers(1, h.size - 4)), int(rng.integers(1, 4))
        h = np.concatenate([h[:pos], bases(rng, n), h[pos:]]) if rng.random() < 0.5 else np.concatenate([h[:pos], h[pos + n:]])
    return h.astype(np.uint8)


def n_reads(r, read_len):
    return max(1, int(round(r["cov"] * r["seq"].size / read_len)))


def case(seed):
    """seed -> dict(seed, k, m, mercy, read_len, err, replicons=[dict(what, seq, circular, cov)], motifs=[names], args=[assemble options])"""
    rng = np.random.default_rng(seed)
    k = int(rng.choice(K_LIST))
    m = int(rng.choice((1, 2, 2, 3)))
    mercy = bool(m > 1 and rng.random() < 0.25)
    read_len = int(rng.choice((k + 1, k + 9, 2 * k + 3, 100, 150)))
    read_len = max(read_len, k + 1)
    err = float(rng.choice(ERRORS))
    backbone = bases(rng, math.exp(rng.uniform(math.log(300), math.log(5000))))
    main_cov = int(rng.choice(COVERAGES))
    inserted, replicons, motifs = [], [], []
    for _ in range(int(rng.integers(0, 7))):
        kind = str(rng.choice(("tandem", "copy", "inverted", "hairpin", "ring", "selfrc-ring", "tip")))
        motifs.append(kind)
        if kind == "tandem":
            period = int(rng.integers(1, k + 6))
            copies = int(rng.integers(2, max(3, 3 * k // period + 1)))
            inserted.append(np.tile(bases(rng, period), copies))
        elif kind in ("copy", "inverted"):
            n = min(int(rng.integers(k - 2, 3 * k + 1)), backbone.size)
            at = int(rng.integers(0, backbone.size - n + 1))
            seg = backbone[at:at + n]
            inserted.append(seg.copy() if kind == "copy" else revcomp(seg))
        elif kind == "hairpin":
            x = bases(rng, rng.integers(k // 2, 2 * k + 1))
            inserted.append(np.concatenate([x, revcomp(x)]))
        elif kind == "ring":
            replicons.append(dict(what=kind, seq=bases(rng, rng.integers(2, 4 * k + 1)), circular=True, cov=int(rng.choice(COVERAGES))))
        elif kind == "selfrc-ring":
            x = bases(rng, rng.integers(1, 2 * k + 1))
            replicons.append(dict(what=kind, seq=np.concatenate([x, revcomp(x)]), circular=True, cov=int(rng.choice(COVERAGES))))
        else:  # a read length of the backbone, then bases of its own: a branch that ends
            at = int(rng.integers(0, max(1, backbone.size - read_len)))
            seq = np.concatenate([backbone[at:at + read_len], bases(rng, rng.integers(1, 3 * k + 1))])
            if rng.random() < 0.5:
                seq = revcomp(seq)  # (the branch runs in as often as out)
            replicons.append(dict(what=kind, seq=seq, circular=False, cov=int(rng.choice(COVERAGES))))
    at = int(rng.integers(0, backbone.size + 1))
    parts = [backbone[:at]]
    for i, x in enumerate(inserted):
        if i:
            parts.append(bases(rng, rng.integers(1, 201)))
        parts.append(x)
    main = np.concatenate(parts + [backbone[at:]]).astype(np.uint8)
    circular = bool(rng.random() < 0.3)
    replicons.insert(0, dict(what="main", seq=main, circular=circular, cov=main_cov))
    if rng.random() < 0.5:
        replicons.insert(1, dict(what="haplotype", seq=second_haplotype(rng, main), circular=circular, cov=main_cov * float(rng.uniform(0.2, 1.0))))
    # the library's size: at most 1.5 M read bases (0.5 M at 3 % errors), by less coverage of every replicon
    cap = 500000 if err >= 0.03 else 1500000
    while True:
        total = sum(n_reads(r, read_len) * read_len for r in replicons)
        if total <= cap:
            break
        for r in replicons:
            r["cov"] = r["cov"] * 0.99 * cap / total
    # assemble
    bubble = int(rng.choice((0, 1, 2), p=(0.2, 0.3, 0.5)))
    prune = int(rng.choice((0, 1, 2, 3), p=(0.2, 0.25, 0.25, 0.3)))
    rounds = int(rng.choice((0, 1, 2, 5), p=(0.1, 0.15, 0.25, 0.5)))
    merge_len, merge_similar = MERGE_PAIRS[int(rng.integers(len(MERGE_PAIRS)))]
    args = ["--bubble_level", str(bubble), "--prune_level", str(prune), "--cleaning_rounds", str(rounds),
            "--min_depth", str(rng.choice(MIN_DEPTHS)), "--max_tip_len", str(int(rng.choice(tip_lens(k)))),
            "--disconnect_ratio", str(rng.choice(DISCONNECT)), "--low_local_ratio", str(rng.choice(LOW_LOCAL)),
            "--min_standalone", str(int(rng.choice((0, k + 1, 200)))), "--merge_len", str(merge_len), "--merge_similar", merge_similar]
    for flag in ("--is_final_round", "--output_standalone", "--careful_bubble"):
        if rng.random() < 0.5:
            args.append(flag)
    return dict(seed=seed, k=k, m=m, mercy=mercy, read_len=read_len, err=err, replicons=replicons, motifs=motifs, args=args)


def reads_of(c):
    """the case's reads: uint8 [n, read_len]; deterministic in the case"""
    rng = np.random.default_rng([c["seed"], 1])
    L, idx, out = c["read_len"], np.arange(c["read_len"]), []
    for r in c["replicons"]:
        seq = r["seq"]
        n = n_reads(r, L)
        if r["circular"]:
            seq = np.tile(seq, -(-(seq.size + L) // seq.size))  # unrolled: a read may start at every base and cross the origin
            start = rng.integers(0, r["seq"].size, size=n)
        elif seq.size < L:
            continue
        else:
            start = rng.integers(0, seq.size - L + 1, size=n)
        reads = seq[start[:, None] + idx[None, :]]
        flip = rng.random(n) < 0.5
        reads[flip] = (3 - reads[flip])[:, ::-1]
        if c["err"] > 0:
            mask = rng.random(reads.shape) < c["err"]
            reads[mask] = (reads[mask] + rng.integers(1, 4, size=int(mask.sum()), dtype=np.uint8)) & 3
        out.append(reads)
    return np.concatenate(out)


def write_library(d, c):
    prefix = os.path.join(d, "reads")
    synth.write_read_lib(prefix, [reads_of(c)], paired=False)
    return prefix


def graph_command(binary, c, lib, g):
    return [binary, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4", "--read_lib_file", lib,
            "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else [])


def max_large_multiplicity(g):
    """the largest edge multiplicity above 254 of graph g, 0 when there is none (its .sdbg files: two bytes per item, the second its
    multiplicity or 255 with the 16-bit value after it, then the label of a tip)"""
    hdr, buckets = canon.canonical_sdbg(g)
    best = 0
    for _, n_items, _, n_large, blob in buckets:
        at = 0
        for _ in range(n_items if n_large else 0):
            tip, mul = blob[at] >> 5 & 1, blob[at + 1]
            at += 2
            if mul == 255:
                best = max(best, blob[at] | blob[at + 1] << 8)
                at += 2
            at += 4 * hdr["words_per_tip_label"] * tip
    return best


def answer(text, out):
    """(digests of the files there are, counts) of one assemble run from its log and its files"""
    log = mbg.parse_log(text)
    log["palindromes"] = int(re.search(r"Graph size without loops: \d+, palindrome: (\d+)", text).group(1))
    for s in (".contigs.fa", ".final.contigs.fa", ".bubble_seq.fa", ".addi.fa"):
        log[s[1:-3].replace(".", "_") + "_records"] = mbg.records(out + s) if os.path.exists(out + s) else 0
    return mpg.digests(out), log


def reference_assemble(g, out, c):
    p = subprocess.run([REF, "assemble", "-s", g, "-o", out, "-t", "1"] + c["args"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=REF_TIMEOUT)
    if p.returncode != 0:
        raise ChildFailed("the reference's assemble", p)
    return answer(p.stderr, out)


def reference_case(c, d):
    """the reference alone: its read2sdbg and its assemble -> (digests, counts, largest multiplicity)"""
    g = os.path.join(d, "g")
    subprocess.run(graph_command(REF, c, write_library(d, c), g), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=REF_TIMEOUT)
    dig, log = reference_assemble(g, os.path.join(d, "ref"), c)
    return dig, log, max_large_multiplicity(g)


def gpu_assemble(g, out, c, d):
    """`mhx_core assemble` on its GPU routes; forwarding to the reference cannot pass"""
    stub = os.path.join(d, "ref_stub.sh")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(stub, 0o755)
    env = dict(os.environ, MHX_REF_CORE=stub, MHX_ASSEMBLE_BUBBLE="1")
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE"):
        env.pop(name, None)
    p = subprocess.run([MHX_CORE, "assemble", "-s", g, "-o", out] + c["args"], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=GPU_TIMEOUT)
    if p.returncode != 0:
        raise ChildFailed("mhx_core assemble", p)
    return answer(p.stderr, out)


def gpu_case(c, d):
    """mhx_core alone: its read2sdbg and its assemble -> (digests, counts)"""
    g = os.path.join(d, "g")
    p = subprocess.run(graph_command(MHX_CORE, c, write_library(d, c), g), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=GPU_TIMEOUT)
    if p.returncode != 0:
        raise ChildFailed("mhx_core read2sdbg", p)
    return gpu_assemble(g, os.path.join(d, "mine"), c, d)


def differences(mine, ref):
    """what differs between two (digests, counts): file names and count names"""
    bad = [s for s in FILES if mine[0].get(s) != ref[0].get(s)]  # (a file only one side wrote differs)
    return bad + [n for n in sorted(set(mine[1]) | set(ref[1])) if mine[1].get(n) != ref[1].get(n)]


def describe(c):
    reps = " ".join("%s%s:%d@%.3g" % (r["what"], "(o)" if r["circular"] else "", r["seq"].size, r["cov"]) for r in c["replicons"])
    return "k %d m %d%s L %d err %g | %s | %s" % (c["k"], c["m"], " mercy" if c["mercy"] else "", c["read_len"], c["err"], reps, " ".join(c["args"]))


def brief(log):
    return "size %d loops %d>%d pal %d tips %d disc %d naive %d complex %d pruned %d final %s bubble_recs %d addi %d contigs %d" % (
        log["graph_size"], log["looped_before"], log["final"]["looped"], log["palindromes"], sum(log["tips"]), sum(log["disconnected"]), sum(log["naive"]),
        sum(log["complex"]), sum(log["pruned"]) + sum(log["more_pruned"]), log["final_pass"], log["bubble_seq_records"], log["addi_records"],
        log["contigs_records"])


def run_one(seed, reference_only, keep):
    """-> None when the case is equal (or ran, with the reference alone), else the text of what went wrong"""
    c = case(seed)
    d = tempfile.mkdtemp(prefix="fuzz_assemble_%d_" % seed)
    t0 = time.time()
    try:
        if reference_only:
            dig, log, mul = reference_case(c, d)
            print("seed %d: %s | %s max_mul %d | %.1f s" % (seed, describe(c), brief(log), mul, time.time() - t0), flush=True)
            return None
        mine = gpu_case(c, d)
        ref = reference_assemble(os.path.join(d, "g"), os.path.join(d, "ref"), c)
        bad = differences(mine, ref)
        print("seed %d: %s | %s | %s" % (seed, describe(c), brief(ref[1]), "differs: " + " ".join(bad) if bad else "equal"), flush=True)
        if bad:
            return "seed %d differs from the reference in %s\n mine: %s\n ref:  %s\n arguments: %s" % (seed, " ".join(bad), mine[1], ref[1], describe(c))
        return None
    except (RuntimeError, subprocess.SubprocessError, OSError) as e:
        print("seed %d: %s" % (seed, describe(c)), flush=True)
        return "seed %d: %s\n arguments: %s" % (seed, e, describe(c))
    finally:
        if keep:
            print("kept: " + d)
        else:
            shutil.rmtree(d, ignore_errors=True)


def committed_cases():
    return [dict(case(seed), name=name) for name, seed in COMMITTED]


def write_golden():
    out = []
    for c in committed_cases():
        d = tempfile.mkdtemp(prefix="fuzz_assemble_")
        try:
            dig, log, mul = reference_case(c, d)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        out.append(dict(name=c["name"], seed=c["seed"], k=c["k"], args=c["args"], digests=dig, log=log, max_mul=mul))
        print(c["name"], brief(log), file=sys.stderr)
    with open(GOLDEN, "w") as f:
        f.write('{"what": "reference megahit_core assemble -t 1 on its own read2sdbg graph of tools/fuzz_assemble.py case(seed)",\n "cases": [\n' +
                ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in out) + "\n ]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seconds", nargs="?", type=float, default=60.0)
    ap.add_argument("seed0", nargs="?", type=int, default=1)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--write-golden", action="store_true")
    a = ap.parse_args()
    if a.write_golden:
        return write_golden()
    if a.seed is not None:
        bad = run_one(a.seed, a.reference_only, keep=True)
        if bad:
            print(bad)
            sys.exit(1)
        return
    t0, n = time.time(), 0
    while time.time() - t0 < a.seconds:
        bad = run_one(a.seed0 + n, a.reference_only, keep=False)
        if bad:  # nothing is started after a failure
            print(bad)
            sys.exit(1)
        n += 1
    dt = time.time() - t0
    print("%d cases in %.1f s (%.2f per second), %s" % (n, dt, n / dt, "the reference alone" if a.reference_only else "all equal to the reference"))


if __name__ == "__main__":
    main()
