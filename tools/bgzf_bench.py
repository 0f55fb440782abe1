"""buildlib on the bench library's reads as FASTQ in BGZF (level 6, 65 280 bytes of text per block: what bgzip writes): wall time of
`mhx_core buildlib` by host zlib (the parent commit's build where --parent-core names one, else this build with the variable unset, which
is the same code path), by the opt-in GPU route (MHX_BUILDLIB_BGZF=1) and on the plain text, on one box and one set of files; the
`bgzf_inflate` / `bgzf_crc` kernel times of MHX_PROFILE=1; compressed and text bytes, blocks.
   python tools/bgzf_bench.py [--reads 1e7] [--parent-core PATH] [--out profiles/NAME.json]"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from megahit_amd import buildid, synth  # noqa: E402

BLOCK = 65280
CHUNK_PAIRS = 65280  # pairs per job: any record width times this is a whole number of blocks


def bgzf_block(text):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    payload = co.compress(text) + co.flush()
    head = b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(payload) + 25)
    return head + payload + struct.pack("<II", zlib.crc32(text), len(text))


def fastq_rows(reads, first, mate, seed):
    """reads uint8 [n, L] of 0..3 -> the FASTQ text of records first .. first + n: '@r<11 digits>/<mate>', the bases, '+', qualities
    binned as current instruments bin them (three values, mostly the highest)"""
    n, L = reads.shape
    W = 16 + L + 1 + 2 + L + 1
    rows = np.empty((n, W), dtype=np.uint8)
    rows[:, 0:2] = np.frombuffer(b"@r", dtype=np.uint8)
    ids = np.arange(first, first + n, dtype=np.int64)
    for d in range(11):
        rows[:, 12 - d] = 48 + (ids // 10 ** d) % 10
    rows[:, 13] = ord("/")
    rows[:, 14] = 48 + mate
    rows[:, 15] = 10
    rows[:, 16:16 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[reads]
    rows[:, 16 + L] = 10
    rows[:, 17 + L] = ord("+")
    rows[:, 18 + L] = 10
    u = np.random.default_rng(seed).random((n, L))
    rows[:, 19 + L:19 + 2 * L] = np.where(u < 0.92, ord("F"), np.where(u < 0.97, ord(":"), ord(","))).astype(np.uint8)
    rows[:, 19 + 2 * L] = 10
    return rows.tobytes()


def job(args):
    """one chunk of pairs -> per mate (text bytes, BGZF bytes, blocks), written to part files"""
    d, i, n_pairs, G, want_text = args
    reads = synth.gen_pe_reads(n_pairs, G, read_len=150, frag=400, err=0.005, seed=1001 + i, genome=synth._genome(1, G))
    out = []
    for mate in (0, 1):
        text = fastq_rows(reads[mate::2], i * CHUNK_PAIRS, mate + 1, 7 * i + mate)
        blocks = [bgzf_block(text[o:o + BLOCK]) for o in range(0, len(text), BLOCK)]
        with open(os.path.join(d, "part%d_%d.gz" % (mate, i)), "wb") as f:
            f.write(b"".join(blocks))
        if want_text:
            with open(os.path.join(d, "part%d_%d.fq" % (mate, i)), "wb") as f:
                f.write(text)
        out.append((len(text), sum(len(b) for b in blocks), len(blocks)))
    return out


def write_library(d, n_reads, procs):
    import multiprocessing as mp
    n_pairs = n_reads // 2
    G = int(n_reads * 2.5)
    jobs = [(d, i, min(CHUNK_PAIRS, n_pairs - lo), G, True) for i, lo in enumerate(range(0, n_pairs, CHUNK_PAIRS))]
    with mp.get_context("spawn").Pool(min(procs, len(jobs))) as pool:
        sizes = pool.map(job, jobs, chunksize=1)
    eof = bgzf_block(b"")
    for mate in (0, 1):
        for ext in ("gz", "fq"):
            with open(os.path.join(d, "r%d.fq%s" % (mate + 1, ".gz" if ext == "gz" else "")), "wb") as f:
                for i in range(len(jobs)):
                    part = os.path.join(d, "part%d_%d.%s" % (mate, i, ext))
                    with open(part, "rb") as g:
                        f.write(g.read())
                    os.remove(part)
                if ext == "gz":
                    f.write(eof)
    for name, ext in (("gz.lib", ".fq.gz"), ("text.lib", ".fq")):
        with open(os.path.join(d, name), "w") as f:
            f.write("bench\npe %s %s\n" % (os.path.join(d, "r1" + ext), os.path.join(d, "r2" + ext)))
    return {"text_bytes": sum(s[m][0] for s in sizes for m in (0, 1)), "compressed_bytes": sum(s[m][1] for s in sizes for m in (0, 1)) + 2 * len(eof),
            "blocks": sum(s[m][2] for s in sizes for m in (0, 1)) + 2}


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blob in iter(lambda: f.read(1 << 24), b""):
            h.update(blob)
    return h.hexdigest()


def timed(exe, lib, out, repeats, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MHX_BUILDLIB")}
    e.update(env)
    best, err = None, ""
    for _ in range(repeats):
        t0 = time.perf_counter()
        p = subprocess.run([exe, "buildlib", lib, out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=e)
        dt = time.perf_counter() - t0
        best, err = (dt if best is None else min(best, dt)), p.stderr
    return round(best, 3), err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=1e7)
    ap.add_argument("--parent-core", default=None, help="mhx_core built from the parent commit (host zlib)")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--gen-only", action="store_true", help="write the files, check them with gzip, run nothing (no GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = int(args.reads) // 2 * 2
    core = os.path.join(ROOT, "megahit_amd", "mhx_core")
    out = {"build_id": buildid.build_id(), "reads": n, "level": 6, "text_bytes_per_block": BLOCK}
    with tempfile.TemporaryDirectory(prefix="mhx_bgzf_") as d:
        t0 = time.perf_counter()
        out.update(write_library(d, n, args.procs))
        out["write_files_s"] = round(time.perf_counter() - t0, 1)
        if args.gen_only:
            import gzip
            for m in (1, 2):
                with gzip.open(os.path.join(d, "r%d.fq.gz" % m), "rb") as f, open(os.path.join(d, "r%d.fq" % m), "rb") as g:
                    assert f.read() == g.read()
            print(json.dumps(out, indent=1))
            return
        p = lambda name: os.path.join(d, name)
        host_exe = args.parent_core or core
        out["host_zlib_is"] = "the parent commit's mhx_core" if args.parent_core else "this build, MHX_BUILDLIB_BGZF unset (the parent's code path)"
        out["host_zlib_s"], _ = timed(host_exe, p("gz.lib"), p("host"), args.repeats)
        out["gpu_bgzf_s"], err = timed(core, p("gz.lib"), p("gpu"), args.repeats, MHX_BUILDLIB_BGZF="1")
        out["route_line"] = (re.search(r"BGZF, \d+ blocks inflated on the GPU", err) or [None])[0]
        if args.parent_core:
            out["this_build_unset_s"], _ = timed(core, p("gz.lib"), p("unset"), 1)
        out["plain_text_s"], _ = timed(core, p("text.lib"), p("text"), args.repeats)
        out["bin_md5"] = {tag: md5(p(tag + ".bin")) for tag in ("host", "gpu", "text")}
        out["identical"] = len(set(out["bin_md5"].values())) == 1 and len({open(p(t + ".lib_info")).read() for t in ("host", "gpu", "text")}) == 1
        prof = p("prof.json")
        _, err = timed(core, p("gz.lib"), p("prof"), 1, MHX_BUILDLIB_BGZF="1", MHX_PROFILE="1", MHX_PROFILE_JSON=prof)
        with open(prof) as f:
            ks = json.load(f)["kernels"]
        out["kernels"] = {k: {"ms": round(v["ms"], 3), "launches": v.get("launches"), "algo_bytes": v["bytes"],
                              "GBs": round(v["bytes"] / v["ms"] / 1e6, 1) if v["ms"] else None}
                          for k, v in sorted(ks.items(), key=lambda kv: -kv[1]["ms"])[:10]}
        m = re.search(r"Device memory: .*", err)
        out["device_memory"] = m.group(0) if m else None
        out["speedup_over_host_zlib"] = round(out["host_zlib_s"] / out["gpu_bgzf_s"], 2)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
