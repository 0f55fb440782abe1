"""`count` through the multi-GPU driver with ONE rank over the RCCL transport, option count_skm_dist at 0 and at 1 in alternating runs
of one process on the bench library (bench.py's reads, k = 21, min count 2) — the way `bench.py --force-dist` runs read2sdbg (GPU).

    python tools/ab_count_skm_dist.py [reads] [runs per setting] [out.json]

One GPU says nothing about the wire: with one rank every exchange is a device copy.  What the figures show is what the route costs an
owner beside the pre-sorted exchange: the records made and ordered, the group-by with its events, the second split of the solid edges."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from megahit_amd import lib  # noqa: E402


def main():
    n_reads = (int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000) // 16 * 16
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    k, m = bench.K, bench.MIN_COUNT
    t0 = time.time()
    packed = bench.make_reads(n_reads, 0, 1)
    print("generated %d reads in %.1f s" % (n_reads, time.time() - t0), file=sys.stderr, flush=True)
    e = lib.Engine(0)
    e.load_sequences(packed, n_reads, bench.READ_LEN, None)
    cm = lib.Comm.rccl(e, lib.comm_unique_id(), 0, 1)
    cm.setup(3, k, m)
    ms, plans, kernels, edges, results = {0: [], 1: []}, {}, {}, {}, {}
    for knob in (0, 1):  # warm-up: allocations, and the two routes' answers against each other
        e.set_option("count_skm_dist", knob)
        res = cm.count(k, m)
        e.synchronize()
        plans[knob] = e.last_s1_plan()
        edges[knob] = e.fetch(lib.BUF_EDGES, np.uint32)
        results[knob] = dict(n_items=int(res.n_items), n_distinct=int(res.n_distinct), n_edges=int(res.n_edges),
                             hist=e.fetch(lib.BUF_MUL_HIST, np.int64), first=e.fetch(lib.BUF_FIRST_0_OUT, np.uint32), last=e.fetch(lib.BUF_LAST_0_IN, np.uint32))
    same = bool(np.array_equal(edges[0], edges[1])) and all(np.array_equal(results[0][n], results[1][n]) for n in ("hist", "first", "last")) and \
        all(results[0][n] == results[1][n] for n in ("n_items", "n_distinct", "n_edges"))
    del edges
    for i in range(runs):
        for knob in (0, 1):
            e.set_option("count_skm_dist", knob)
            last = i == runs - 1
            if last:
                e.profile(True)
                e.profile_reset()
            e.synchronize()
            t = time.perf_counter()
            cm.count(k, m)
            e.synchronize()
            ms[knob].append((time.perf_counter() - t) * 1e3)
            if last:
                kernels[knob] = {n: round(v["ms"], 3) for n, v in sorted(e.profile_get().items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] >= 0.05}
                e.profile(False)
    out = {"what": "mhx_dist_count, one rank over the RCCL transport, count_skm_dist 0 / 1 alternating in one process", "reads": n_reads, "read_len": bench.READ_LEN,
           "k": k, "min_count": m, "runs_per_setting": runs, "same_results": same, "n_edges": results[0]["n_edges"]}
    for knob in (0, 1):
        out["count_skm_dist=%d" % knob] = {"plan": plans[knob], "ms": [round(x, 2) for x in ms[knob]], "median_ms": round(statistics.median(ms[knob]), 2),
                                           "spread_ms": round(max(ms[knob]) - min(ms[knob]), 2), "kernels_ms_profiled_run": kernels[knob]}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    cm.close()
    e.close()
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
