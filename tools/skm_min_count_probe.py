"""GPU probe: min count 3 and 4 on super-k-mer records (s1_skm_max_m = 4) against the prefix plan that serves them without the knob
(s1_skm_max_m = 2: the parent's route).  The 10 M x 150 bp library of bench.py, k = 21, min count 3 and 4, read2sdbg (stage 1 + stage 2)
and count, one process; the two settings in turn, block by block: two warm-up steps each, then blocks of one untimed step (the arrays of
the other route are sized anew) and three timed ones, twice — six timed steps a setting, wall clock around a synchronised step — and two
more steps under the library's profile (device events around every launch) for the per-kernel times and their sum.  The SdBG digest and the
edge digest must be equal between the settings; the plan line of the new route says how many rounds took the second look.

    python tools/skm_min_count_probe.py [reads] > profiles/r17_skm_min_count.json"""
import hashlib
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from megahit_amd import lib  # noqa: E402
from megahit_amd.buildid import build_id, lib_id  # noqa: E402

K, BLOCKS, TIMED, PROFILED = bench.K, 2, 3, 2


def main():
    pos = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_reads = (int(float(pos[0])) if pos else 10000000) // 16 * 16
    packed = bench.make_reads(n_reads, 0, 1)
    eng = lib.Engine(0)
    eng.load_sequences(packed, n_reads, bench.READ_LEN, None)

    def digest(bufs):
        h = hashlib.md5()
        for b, t in bufs:
            h.update(eng.fetch(b, t).tobytes())
        return h.hexdigest()

    def step(engine_name, m):
        if engine_name == "count":
            eng.count(K, m)
            return eng.last_s1_plan()
        eng.read2sdbg_s1(K, m)
        plan = eng.last_s1_plan()
        eng.read2sdbg_s2(K, m)
        return plan

    out = {"build_id": build_id(), "lib_id": lib_id(), "reads": n_reads, "read_len": bench.READ_LEN, "k": K, "timed_steps": BLOCKS * TIMED, "warmup": 2, "runs": [],
           "digests_equal": True}
    try:
        for m in (3, 4):
            for engine_name in ("read2sdbg", "count"):
                rows = {}
                for knob in (2, 4):
                    eng.set_option("s1_skm_max_m", knob)
                    for _ in range(2):
                        step(engine_name, m)
                    eng.synchronize()
                    rows[knob] = {"ms": []}
                for _ in range(BLOCKS):
                    for knob in (2, 4):
                        eng.set_option("s1_skm_max_m", knob)
                        step(engine_name, m)
                        eng.synchronize()
                        for _ in range(TIMED):
                            t0 = time.perf_counter()
                            step(engine_name, m)
                            eng.synchronize()
                            rows[knob]["ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                for knob in (2, 4):
                    eng.set_option("s1_skm_max_m", knob)
                    step(engine_name, m)
                    eng.synchronize()
                    eng.profile(True)
                    eng.profile_reset()
                    for _ in range(PROFILED):
                        plan = step(engine_name, m)
                    eng.synchronize()
                    st = eng.profile_get()
                    eng.profile(False)
                    if engine_name == "count":
                        d = digest(((lib.BUF_EDGES, np.uint32), (lib.BUF_BUCKET_COUNT, np.uint64), (lib.BUF_MUL_HIST, np.int64), (lib.BUF_FIRST_0_OUT, np.uint32),
                                    (lib.BUF_LAST_0_IN, np.uint32)))
                    else:
                        d = digest(((lib.BUF_SDBG_BYTES, np.uint8), (lib.BUF_BUCKET_COUNT, np.uint64), (lib.BUF_BUCKET_TIPS, np.uint64), (lib.BUF_IS_SOLID, np.uint64),
                                    (lib.BUF_MUL_HIST, np.int64)))
                    ms = rows[knob]["ms"]
                    look = re.search(r"a second look in (\d+) of (\d+) rounds", plan)
                    groups = "count_skm_groups" if engine_name == "count" else "s1_skm_groups"
                    rows[knob] = {"engine": engine_name, "min_count": m, "s1_skm_max_m": knob, "route": "super-k-mer records" if "super-k-mers" in plan[:30] else "prefix plan",
                                  "ms_per_step": round(sum(ms) / len(ms), 3), "ms_steps": ms, "spread_ms": round(max(ms) - min(ms), 3),
                                  "kernels_ms_per_step": round(sum(v["ms"] for v in st.values()) / PROFILED, 3),
                                  "groups_kernel_ms_per_step": round(st[groups]["ms"] / PROFILED, 3) if groups in st else None,
                                  "second_look_rounds": [int(look.group(1)), int(look.group(2))] if look else None, "plan": plan, "digest": d,
                                  "kernel_ms_per_step": {k: round(v["ms"] / PROFILED, 3) for k, v in sorted(st.items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] / PROFILED > 0.3}}
                    print("m %d | %s | s1_skm_max_m %d: %.3f ms (%s)" % (m, engine_name, knob, rows[knob]["ms_per_step"], plan[:70]), file=sys.stderr, flush=True)
                equal = rows[2]["digest"] == rows[4]["digest"]
                out["digests_equal"] = out["digests_equal"] and equal
                out["runs"] += [rows[2], rows[4]]
                if not equal:
                    print("*** digests differ: m %d %s" % (m, engine_name), file=sys.stderr, flush=True)
    finally:
        eng.set_option("s1_skm_max_m", 2)
    print(json.dumps(out, indent=1))
    sys.exit(0 if out["digests_equal"] else 1)


if __name__ == "__main__":
    main()
