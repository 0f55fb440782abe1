"""The unitig graph at bench size: 10 M x 150 bp PE reads of one genome (2.5 bp per read, 0.5 % errors: the bench.py
workload family, synth.gen_shard_library), graph by `mhx_core read2sdbg -k 21 -m 2`, then `mhx_core assemble
--bubble_level 0 --prune_level 0 --cleaning_rounds 0` with MHX_PROFILE=1 (per-kernel times of links / ranking / vertices /
text), and the reference's `megahit_core assemble` on the same graph at -t 1 and -t 16: wall times and the digest of
.contigs.fa (equal to ours at -t 1); the wall time of mhx_core again --wall-runs times without MHX_PROFILE.  --clean: the same with `--cleaning_rounds 5` and MHX_ASSEMBLE_CLEAN=1 (the weak-link
and tip rounds on the device: the clean_* kernel groups), the reference's cleaning time summed from its per-step log lines.
--prune: `--prune_level 2 --min_depth 2 --cleaning_rounds 5` and MHX_ASSEMBLE_PRUNE=1 (what an unmodified `megahit --bubble-level 0`
asks for; the low-depth passes are the clean_low_depth group, their number its launches), the digests of .contigs.fa and .addi.fa.
--bubble: `--bubble_level 2 --prune_level 2 --min_depth 2 --merge_len 20 --merge_similar 0.95 --cleaning_rounds 5 --careful_bubble`
and MHX_ASSEMBLE_BUBBLE=1 (what an unmodified `megahit` asks for below k_max; the kernel groups clean_bubbles and clean_similarity,
the per-round bubble counts, the mid-run finishes), the digests of .contigs.fa, .addi.fa and .bubble_seq.fa.  --diploid F: a second
haplotype (an SNP, an SNP pair, a 1-3 base deletion, a 1-3 base insertion in turn, one every 1000 bases of the genome:
make_unitig_bubble_golden.second_haplotype) sampled by F x as many extra reads, so that the graph holds bubbles of both kinds.
--infer (with --prune or --bubble): without `--min_depth` and the route's variable at 2, so that the route infers it on the device; "infer_ms" = the kernel groups
sdbg_mul_hist and sdbg_pack of the profiled run.
Too slow for the suite.  One JSON line on stdout.

    python tools/unitig_bench.py [--clean | --prune | --bubble] [--infer] [--diploid 0.5] [--reads 10000000] [--ref oracle/_ref/ref_megahit_core] [--ref-threads 1,16] [--workdir DIR]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from megahit_amd import synth  # noqa: E402

MHX_CORE = os.path.join(ROOT, "megahit_amd", "mhx_core")
QUAL = ["--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"]


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    ap.add_argument("--ref-threads", default="1,16")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--wall-runs", type=int, default=5, help="runs of mhx_core assemble without MHX_PROFILE for the wall time")
    ap.add_argument("--clean", action="store_true", help="--cleaning_rounds 5 on the GPU route (MHX_ASSEMBLE_CLEAN=1)")
    ap.add_argument("--prune", action="store_true", help="--prune_level 2 --min_depth 2 --cleaning_rounds 5 on the GPU route (MHX_ASSEMBLE_PRUNE=1)")
    ap.add_argument("--bubble", action="store_true", help="bubble level 2, prune level 2, careful, on the GPU route (MHX_ASSEMBLE_BUBBLE=1)")
    ap.add_argument("--infer", action="store_true", help="with --prune / --bubble: no --min_depth, so the route infers it (kernel group sdbg_mul_hist)")
    ap.add_argument("--diploid", type=float, default=0.0, help="add this fraction of the reads again from a second haplotype (a variant every 1000 bases)")
    a = ap.parse_args()
    qual = QUAL[:-1] + ["5"] if a.clean else QUAL
    if a.prune:
        qual = ["--bubble_level", "0", "--prune_level", "2", "--min_depth", "2", "--cleaning_rounds", "5"]
    if a.bubble:
        qual = ["--bubble_level", "2", "--prune_level", "2", "--min_depth", "2", "--merge_len", "20", "--merge_similar", "0.95", "--cleaning_rounds", "5",
                "--careful_bubble"]
    if a.infer:
        at = qual.index("--min_depth")
        qual = qual[:at] + qual[at + 2:]
    d = a.workdir or tempfile.mkdtemp(prefix="mhx_unitig")
    os.makedirs(d, exist_ok=True)
    res = {"reads": a.reads, "k": a.k, "options": " ".join(qual)}
    genome, blocks = synth.gen_shard_library(a.reads, 1, 1001)
    if a.diploid > 0:
        import numpy as np
        import make_unitig_bubble_golden as mbg
        h = mbg.second_haplotype(np.asarray(genome, dtype=np.uint8), dict(seed=1001, gap=1000, near=8))
        n_extra = int(a.reads * a.diploid) // 2
        blocks = list(blocks) + [synth.gen_pe_reads(n_extra, h.size, read_len=blocks[0].shape[1], frag=400, err=0.005, seed=1003, genome=h)]
        res["diploid"] = a.diploid
    synth.write_read_lib(os.path.join(d, "reads"), blocks)
    g = os.path.join(d, "g")
    subprocess.run([MHX_CORE, "read2sdbg", "-k", str(a.k), "-m", "2", "--host_mem", "2e10", "--num_cpu_threads", "16", "--read_lib_file",
                    os.path.join(d, "reads"), "--output_prefix", g], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    level = "2" if a.infer else "1"  # 2: a command line without a depth is served
    env = dict(os.environ, MHX_PROFILE="1", MHX_SERVER="off", MHX_ASSEMBLE_CLEAN="1" if a.clean else "0", MHX_ASSEMBLE_PRUNE=level if a.prune else "0",
               MHX_ASSEMBLE_BUBBLE=level if a.bubble else "0")
    t0 = time.time()
    p = subprocess.run([MHX_CORE, "assemble", "-s", g, "-o", os.path.join(d, "mine"), "-t", "16"] + qual, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, check=True)
    res["mhx_wall_s"] = round(time.time() - t0, 3)
    res["kernels_ms"] = {m.group(1): float(m.group(2)) for m in re.finditer(r"profile (\S+)\s+\d+ launches\s+([\d.]+) ms", p.stderr)}
    res["log"] = [l for l in p.stderr.splitlines() if re.search(r"Edges|Tips|unitig graph size|palindrome|Max:|output|disconnected|pruning|low depth|ubble|min depth", l)]
    res["mhx_digest"] = md5(os.path.join(d, "mine.contigs.fa"))
    if a.prune:
        m = re.search(r"profile clean_low_depth\s+(\d+) launches", p.stderr)
        res["low_depth_passes"] = int(m.group(1)) if m else None
        res["mhx_addi_digest"] = md5(os.path.join(d, "mine.addi.fa"))
    if a.infer:  # the histogram kernel beside k_sdbg_pack, which reads the same multiplicities (same profiled run)
        res["infer_ms"] = {g_: res["kernels_ms"].get(g_) for g_ in ("sdbg_mul_hist", "sdbg_pack")}
    if a.bubble:
        res["mhx_addi_digest"] = md5(os.path.join(d, "mine.addi.fa"))
        res["mhx_bubble_seq_digest"] = md5(os.path.join(d, "mine.bubble_seq.fa"))
        res["bubble_groups_ms"] = {g_: res["kernels_ms"].get(g_) for g_ in ("clean_bubbles", "clean_similarity")}
    # the wall time files to files with the profiler off (the events of MHX_PROFILE serialise the launches): every run listed
    env.pop("MHX_PROFILE")
    walls = []
    for _ in range(a.wall_runs):
        t0 = time.time()
        subprocess.run([MHX_CORE, "assemble", "-s", g, "-o", os.path.join(d, "mine"), "-t", "16"] + qual, env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, check=True)
        walls.append(round(time.time() - t0, 3))
    res["mhx_wall_unprofiled_s"] = walls
    if os.path.exists(a.ref):
        for t in [int(x) for x in a.ref_threads.split(",") if x]:
            out = os.path.join(d, "ref_t%d" % t)
            t0 = time.time()
            q = subprocess.run([a.ref, "assemble", "-s", g, "-o", out, "-t", str(t)] + qual, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               text=True, check=True)
            res["ref_t%d_wall_s" % t] = round(time.time() - t0, 3)
            m = re.search(r"unitig graph size: \d+, time for building: ([\d.]+)", q.stderr)
            res["ref_t%d_unitig_s" % t] = float(m.group(1)) if m else None
            m = re.search(r"Tips removal done! Time elapsed\(sec\): ([\d.]+)", q.stderr)
            res["ref_t%d_tips_s" % t] = float(m.group(1)) if m else None
            m = re.search(r"Time to output: ([\d.]+)", q.stderr)
            res["ref_t%d_output_s" % t] = float(m.group(1)) if m else None
            if a.clean:  # "Tips removed: N, time: T" and "Number unitigs disconnected: N, time: T" of every round
                res["ref_t%d_cleaning_s" % t] = round(sum(float(x) for x in re.findall(r"(?:Tips removed|disconnected): \d+, time: ([\d.]+)", q.stderr)), 3)
                res["ref_t%d_rounds" % t] = re.findall(r"(?:Tips removed|disconnected): (\d+)", q.stderr)
            if a.prune:
                res["ref_t%d_cleaning_s" % t] = round(sum(float(x) for x in re.findall(r"(?:Tips removed|disconnected|excessive pruning): \d+, time: ([\d.]+)",
                                                                                      q.stderr)), 3)
                res["ref_t%d_rounds" % t] = re.findall(r"(?:Tips removed|disconnected|excessive pruning): (\d+)", q.stderr)
                m = re.search(r"local low depth unitigs removed: (\d+), complex bubbles removed: 0, time: ([\d.]+)", q.stderr)
                res["ref_t%d_low_depth" % t] = [int(m.group(1)), float(m.group(2))] if m else None
            if t == 1:
                res["ref_t1_digest"] = md5(out + ".contigs.fa")
                res["digest_equal"] = res["ref_t1_digest"] == res["mhx_digest"]
                if a.prune or a.bubble:
                    res["addi_digest_equal"] = md5(out + ".addi.fa") == res["mhx_addi_digest"]
                if a.bubble:
                    res["bubble_seq_digest_equal"] = md5(out + ".bubble_seq.fa") == res["mhx_bubble_seq_digest"]
            if a.bubble:
                res["ref_t%d_rounds" % t] = re.findall(r"(?:Tips removed|disconnected|bubbles removed|excessive pruning): (\d+)", q.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
