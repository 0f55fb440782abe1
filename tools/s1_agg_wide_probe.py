"""GPU probe: read2sdbg at k = 27 and k = 23, min count 2, with stage 1 leaving stage 2's aggregated items (s1_agg_wide = 1) against stage 2
from a count of the (k+1)-mers behind a stage 1 without items (s1_agg_wide = 0: the default route).  The 10 M x 150 bp library of bench.py,
one process; the two settings in turn, block by block: two warm-up steps each, then blocks of one untimed step (the arrays of the other
route are sized anew) and three timed ones, twice — six timed steps a setting, wall clock around a synchronised step — and two more steps
under the library's profile (device events around every launch), stage 1 and stage 2 apart, for the per-kernel times and their sums.  The
SdBG digests must be equal between the settings.  Then two ranks as threads on this device (1 M reads each, in-process transport):
mhx_comm_bytes_sent over mhx_dist_read2sdbg both ways — stage 1's exchange is the same, the difference is stage 2's.

    python tools/s1_agg_wide_probe.py [reads] > profiles/r20_s1_agg_wide.json"""
import hashlib
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from megahit_amd import lib  # noqa: E402
from megahit_amd.buildid import build_id, lib_id  # noqa: E402

M, BLOCKS, TIMED, PROFILED = 2, 2, 3, 2
MARKER = "[aggregated stage-2 items"


def single_gpu(n_reads, out):
    packed = bench.make_reads(n_reads, 0, 1)
    eng = lib.Engine(0)
    eng.load_sequences(packed, n_reads, bench.READ_LEN, None)

    def step(k):
        eng.read2sdbg_s1(k, M)
        plan = eng.last_s1_plan()
        eng.read2sdbg_s2(k, M)
        return plan

    def profiled(k):
        """-> plan, per-kernel ms of stage 1 and of stage 2, summed over PROFILED steps"""
        s1, s2, plan = {}, {}, ""
        eng.profile(True)
        for _ in range(PROFILED):
            eng.profile_reset()
            eng.read2sdbg_s1(k, M)
            eng.synchronize()
            plan = eng.last_s1_plan()
            for n, v in eng.profile_get().items():
                s1[n] = s1.get(n, 0.0) + v["ms"]
            eng.profile_reset()
            eng.read2sdbg_s2(k, M)
            eng.synchronize()
            for n, v in eng.profile_get().items():
                s2[n] = s2.get(n, 0.0) + v["ms"]
        eng.profile(False)
        return plan, s1, s2

    try:
        for k in (27, 23):
            rows = {}
            for knob in (0, 1):
                eng.set_option("s1_agg_wide", knob)
                for _ in range(2):
                    step(k)
                eng.synchronize()
                rows[knob] = {"ms": []}
            for _ in range(BLOCKS):
                for knob in (0, 1):
                    eng.set_option("s1_agg_wide", knob)
                    step(k)
                    eng.synchronize()
                    for _ in range(TIMED):
                        t0 = time.perf_counter()
                        step(k)
                        eng.synchronize()
                        rows[knob]["ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
            for knob in (0, 1):
                eng.set_option("s1_agg_wide", knob)
                step(k)
                eng.synchronize()
                plan, s1, s2 = profiled(k)
                h = hashlib.md5()
                for b, t in ((lib.BUF_SDBG_BYTES, np.uint8), (lib.BUF_BUCKET_COUNT, np.uint64), (lib.BUF_BUCKET_TIPS, np.uint64), (lib.BUF_IS_SOLID, np.uint64),
                             (lib.BUF_MUL_HIST, np.int64)):
                    h.update(eng.fetch(b, t).tobytes())
                ms = rows[knob]["ms"]

                def top(st):
                    return {n: round(v / PROFILED, 3) for n, v in sorted(st.items(), key=lambda kv: -kv[1]) if v / PROFILED > 0.3}

                rows[knob] = {"k": k, "min_count": M, "s1_agg_wide": knob, "items_from_stage_1": MARKER in plan, "ms_per_step": round(sum(ms) / len(ms), 3), "ms_steps": ms,
                              "spread_ms": round(max(ms) - min(ms), 3), "stage_1_kernels_ms": round(sum(s1.values()) / PROFILED, 3),
                              "stage_2_kernels_ms": round(sum(s2.values()) / PROFILED, 3),
                              "s1_groups_ms": round((s1.get("s1_groups", 0.0) + s1.get("s1_giant_groups", 0.0)) / PROFILED, 3), "plan": plan, "digest": h.hexdigest(),
                              "stage_1_kernel_ms": top(s1), "stage_2_kernel_ms": top(s2)}
                print("k %d | s1_agg_wide %d: %.3f ms a step, stage 1 %.3f + stage 2 %.3f ms of kernels (%s)" %
                      (k, knob, rows[knob]["ms_per_step"], rows[knob]["stage_1_kernels_ms"], rows[knob]["stage_2_kernels_ms"], plan[-60:]), file=sys.stderr, flush=True)
            equal = rows[0]["digest"] == rows[1]["digest"]
            out["digests_equal"] = out["digests_equal"] and equal
            out["runs"] += [rows[0], rows[1]]
            if not equal:
                print("*** digests differ: k %d" % k, file=sys.stderr, flush=True)
    finally:
        eng.set_option("s1_agg_wide", 0)
        eng.close()


def two_ranks(n_reads, out):
    """bytes on the wire of mhx_dist_read2sdbg at world 2, k = 27, both ways (recorded, not judged: at min count 2 a key with exactly two
    occurrences makes as many items as occurrences)"""
    world, k = 2, 27
    for knob in (0, 1):
        engines = [lib.Engine(0) for _ in range(world)]
        for r, e in enumerate(engines):
            e.set_option("s1_agg_wide", knob)
            e.load_sequences(bench.make_reads(n_reads, r, world), n_reads, bench.READ_LEN, None)
        comms = lib.Comm.local_group(engines)
        res, err = [None] * world, [None] * world

        def work(r):
            try:
                comms[r].setup(0, k, M)
                comms[r].bytes_sent(reset=True)
                comms[r].read2sdbg(k, M)
                res[r] = (comms[r].bytes_sent(), engines[r].last_s1_plan(), hashlib.md5(engines[r].fetch(lib.BUF_SDBG_BYTES, np.uint8).tobytes()).hexdigest())
            except BaseException as ex:  # noqa: BLE001 - re-raised below
                err[r] = ex

        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=600)
        for cm in comms:
            cm.close()
        for e in engines:
            e.close()
        for ex in err:
            if ex is not None:
                raise ex
        out["two_ranks"].append({"k": k, "min_count": M, "reads_per_rank": n_reads, "s1_agg_wide": knob, "bytes_sent": [x[0] for x in res],
                                 "items_from_stage_1": [MARKER in x[1] for x in res], "digests": [x[2] for x in res]})
    a, b = out["two_ranks"][-2:]
    out["digests_equal"] = out["digests_equal"] and a["digests"] == b["digests"]


def main():
    pos = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_reads = (int(float(pos[0])) if pos else 10000000) // 16 * 16
    out = {"build_id": build_id(), "lib_id": lib_id(), "reads": n_reads, "read_len": bench.READ_LEN, "timed_steps": BLOCKS * TIMED, "warmup": 2, "runs": [],
           "two_ranks": [], "digests_equal": True}
    single_gpu(n_reads, out)
    two_ranks(min(n_reads, 1000000) // 16 * 16, out)
    print(json.dumps(out, indent=1))
    sys.exit(0 if out["digests_equal"] else 1)


if __name__ == "__main__":
    main()
