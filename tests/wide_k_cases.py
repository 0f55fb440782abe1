"""Inputs of the wide-k sweep (test_gpu_wide_k*.py, test_wide_k_golden_file.py, test_oracle_vs_ref.py, tools/make_wide_k_golden.py):
one seeded read library per k, and the k at which a key, record, edge or tip-label width begins or ends (9 <= k <= 255)."""
import os
import subprocess

import numpy as np

from megahit_amd import canon, synth

SEED = 7
COMMON = ["--host_mem", "2e9", "--num_cpu_threads", "3"]


def library(seed, k, n_pairs=400, genome_len=4000, read_len=300):
    """~200 kb: paired reads of 300 bases (longer than 256) with every third cut to 0..300 bases, three copies each of the prefixes
    of k-1 .. k+3 bases of one random sequence and of their reverse complements (every read-length edge around k), poly-A,
    (AT)n (its own reverse complement) and (AC)n reads (hot keys), one empty read"""
    rng = np.random.default_rng(seed)
    r = synth.gen_pe_reads(n_pairs, genome_len, read_len=read_len, frag=500, err=0.004, seed=seed)
    out = [x[: int(rng.integers(0, read_len + 1))] if i % 3 == 0 else x for i, x in enumerate(r)]
    g = rng.integers(0, 4, size=600, dtype=np.uint8)
    for n in (k - 1, k, k + 1, k + 2, k + 3):
        for _ in range(3):
            out.append(g[:n].copy())
            out.append((3 - g[:n][::-1]).astype(np.uint8))
    out += [np.zeros(300, dtype=np.uint8) for _ in range(6)]
    out += [np.tile(np.array([0, 3], dtype=np.uint8), 150) for _ in range(6)]
    out += [np.tile(np.array([0, 1], dtype=np.uint8), 150)[:299] for _ in range(5)]
    out.append(np.zeros(0, dtype=np.uint8))
    return out


def fixed_library(seed, k):
    """the 300-base reads of library(seed, k) only: a read set of one length"""
    return [r for r in library(seed, k) if len(r) == 300]


def s1_kw(k):
    """words of the stage-1 key (and, by the same formula, of the stage-2 key)"""
    return (2 * k + 4 + 31) // 32


def s1_stride(k):
    """words of a non-compact stage-1 record: key + two words, rounded up to even (s1_stride of s1.hip)"""
    return (s1_kw(k) + 2 + 1) // 2 * 2


def edge_words(k):
    return (2 * k + 18 + 31) // 32


# 16j-3: the last k of a stage-1 / stage-2 key width; 16j-1: the first k of the next (k + 1 a multiple of 16);
# 16j+1: the first k of a tip-label and sequence-word width
K_ALL = sorted({9, 11, 253, 255} | {16 * j + d for j in range(1, 16) for d in (-3, -1, 1)})
# the last and the first k of each edge-record width (count only)
K_EDGE_WORDS = sorted({16 * j + d for j in range(1, 16) for d in (7, 9)})
# the widest k of each record stride 4, 6, ..., 20 of non-compact stage 1
K_STRIDES = [max(k for k in range(9, 256, 2) if s1_stride(k) == s) for s in range(4, 21, 2)]
# the only k >= 45 of K_ALL at which the oracle finds no mercy edge for seq2sdbg in library(SEED, k) (at most two are allowed)
GEN_MERCY_ZERO = (191, 193)
K_GOLDEN = (45, 63, 95, 127, 191, 255)

assert len(K_ALL) == 49 and len(K_EDGE_WORDS) == 30 and all(k % 2 == 1 and 9 <= k <= 255 for k in K_ALL + K_EDGE_WORDS)
assert [s1_stride(k) for k in K_STRIDES] == list(range(4, 21, 2)) and K_STRIDES[-1] == 255
assert len(GEN_MERCY_ZERO) <= 2


def write_library(workdir, seed, k, fixed=False):
    prefix = os.path.join(workdir, "reads")
    synth.write_read_lib(prefix, [fixed_library(seed, k) if fixed else library(seed, k)])
    return prefix


def run_four(binary, lib_prefix, k, workdir, m=2):
    """count, seq2sdbg --need_mercy on its edges, read2sdbg and read2sdbg --need_mercy of a megahit_core-compatible binary ->
    the digests and record counts that tests/golden/wide_k.json holds for one k, and the prefixes of the three SdBGs"""
    cnt, sd, o, om = (os.path.join(workdir, x) for x in ("cnt", "sdbg", "out", "outm"))

    def call(args):
        p = subprocess.run([binary] + args + COMMON, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, "%s %s: %s" % (os.path.basename(binary), " ".join(args[:3]), p.stderr[-2000:])

    call(["count", "-k", str(k), "-m", str(m), "--read_lib_file", lib_prefix, "--output_prefix", cnt])
    call(["seq2sdbg", "-k", str(k), "--kmer_from", "0", "--input_prefix", cnt, "--output_prefix", sd, "--need_mercy"])
    call(["read2sdbg", "-k", str(k), "-m", str(m), "--read_lib_file", lib_prefix, "--output_prefix", o])
    call(["read2sdbg", "-k", str(k), "-m", str(m), "--read_lib_file", lib_prefix, "--output_prefix", om, "--need_mercy"])

    def n_sdbg(prefix):
        return int(sum(b[1] for b in canon.canonical_sdbg(prefix)[1]))

    got = {"k": k, "m": m, "edges": canon.digest_edges(cnt), "n_edges": int(canon.canonical_edges(cnt)[1].shape[0]),
           "cand": canon.digest_file(cnt + ".cand"), "counting": canon.digest_file(cnt + ".counting"),
           "seq2sdbg_mercy": canon.digest_sdbg(sd), "n_seq2sdbg_mercy": n_sdbg(sd),
           "read2sdbg": canon.digest_sdbg(o), "n_read2sdbg": n_sdbg(o),
           "read2sdbg_mercy": canon.digest_sdbg(om), "n_read2sdbg_mercy": n_sdbg(om)}
    return got, {"seq2sdbg_mercy": sd, "read2sdbg": o, "read2sdbg_mercy": om}
