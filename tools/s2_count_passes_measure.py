"""Stage 2 from a count in passes against the per-occurrence lv1 passes, at size (profiles/r18_s2_count_passes.json).

`mhx_core read2sdbg -k 27 -m 1` on the synthetic metagenome library of tools/make_fullsize_golden.py (--reads, default the 40 M-read
shard of tests/test_gpu_fullsize_meta.py), with the free device memory faked to --factor bytes per base — 38 fails the once-fit of
stage 2 from a count by one per cent at that size (13 B x 2.2 estimated items per base x 17/16 = 30.4 per base against 0.8 of the
free bytes less two staging batches of 1 GiB: 30.0) —, 0: the real free memory.  Runs --runs times each:

  * --parent-core (an mhx_core built from the parent commit, beside its own libmhx.so): the per-occurrence lv1 passes;
  * this tree's mhx_core (MHX_S2_COUNT_PASSES=1, its default): the count in passes;

and records per run the wall time, the summed kernel time (MHX_PROFILE), the passes, the peak device bytes of stage 2 and the digest
(compared with tests/golden/fullsize_meta.json at 40 M reads).

    python tools/s2_count_passes_measure.py --out profiles/r18_s2_count_passes.json [--parent-core PATH] [--reads 62500000 --factor 0]
"""
import argparse
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
from megahit_amd import canon  # noqa: E402
import make_fullsize_golden as mfg  # noqa: E402

CORE = os.path.join(ROOT, "megahit_amd", "mhx_core")
K, M = 27, 1


def one_run(core, lib, out, env):
    t0 = time.time()
    p = subprocess.run([core, "read2sdbg", "-k", str(K), "-m", str(M), "--host_mem", "64e9", "--num_cpu_threads", "8", "--read_lib_file", lib, "--output_prefix", out],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=dict(os.environ, MHX_PROFILE="1", **env), timeout=900)
    wall = time.time() - t0
    if p.returncode != 0:
        raise SystemExit("exit %d\n%s" % (p.returncode, p.stderr[-3000:]))
    err = p.stderr
    kernels = {m.group(1): (int(m.group(2)), float(m.group(3))) for m in re.finditer(r"profile (\S+)\s+(\d+) launches\s+([0-9.]+) ms", err)}
    lv1 = re.search(r"Memory plan: (\d+) passes over lv1 bucket ranges", err)
    own = re.search(r"Memory plan: stage 2 from a count in (\d+) passes over its own bucket ranges[^\n]*", err)
    mem = re.search(r"Device memory of stage 2: (\d+) bytes held when planned, peak (\d+) bytes, budget (\d+)", err)
    res = {"wall_s": round(wall, 3), "kernels_ms": round(sum(v[1] for v in kernels.values()), 1),
           "top_kernels_ms": {n: round(v[1], 1) for n, v in sorted(kernels.items(), key=lambda kv: -kv[1][1])[:8]},
           "lv1_passes": int(lv1.group(1)) if lv1 else 1, "count_passes": int(own.group(1)) if own else 0, "plan_line": own.group(0) if own else (lv1.group(0) if lv1 else ""),
           "given_up": "given up" in err, "digest": canon.digest_sdbg(out)}
    if mem:
        res.update(held_when_planned=int(mem.group(1)), peak_bytes=int(mem.group(2)), budget=int(mem.group(3)))
    for fn in os.listdir(os.path.dirname(out)):
        if fn.startswith(os.path.basename(out)):
            os.remove(os.path.join(os.path.dirname(out), fn))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=mfg.META["reads"])
    ap.add_argument("--factor", type=float, default=38.0, help="MHX_FREE_BYTES per base of the library; 0: the real free memory")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-core", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_s2_count_passes.json"))
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    n_reads = int(a.reads) // 2 * 2
    d = a.dir or tempfile.mkdtemp(prefix="mhx_s2cp_")
    lib = os.path.join(d, "reads")
    if not os.path.exists(lib + ".bin"):
        mfg.gen_meta_library(lib, n_reads)
    with open(lib + ".lib_info") as f:
        bases = int(f.read().split()[0])
    env = {"MHX_FREE_BYTES": str(int(a.factor * bases))} if a.factor else {}
    result = {"reads": n_reads, "bases": bases, "k": K, "m": M, "factor": a.factor, "MHX_FREE_BYTES": env.get("MHX_FREE_BYTES", "not set: the real free memory"), "runs": {}}
    gold_path = os.path.join(ROOT, "tests", "golden", "fullsize_meta.json")
    if os.path.exists(gold_path):
        with open(gold_path) as f:
            gold = json.load(f)
        if gold["reads"] == n_reads:
            result["golden_digest"] = gold["cases"]["read2sdbg"]["digest"]
    routes = ([("parent: per-occurrence lv1 passes", a.parent_core, {})] if a.parent_core else []) + [("count in passes (MHX_S2_COUNT_PASSES=1)", CORE, {"MHX_S2_COUNT_PASSES": "1"})]
    for label, core, extra in routes:
        result["runs"][label] = []
        for i in range(a.runs):
            r = one_run(core, lib, os.path.join(d, "out"), dict(env, **extra))
            print(label, i, json.dumps(r), flush=True)
            result["runs"][label].append(r)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    for label, runs in result["runs"].items():
        walls, kern = [r["wall_s"] for r in runs], [r["kernels_ms"] for r in runs]
        result.setdefault("summary", {})[label] = {"wall_s_min_max": [min(walls), max(walls)], "kernels_ms_min_max": [min(kern), max(kern)],
                                                   "digest_is_golden": all(r["digest"] == result.get("golden_digest", r["digest"]) for r in runs)}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result.get("summary", {}), indent=1))


if __name__ == "__main__":
    main()
