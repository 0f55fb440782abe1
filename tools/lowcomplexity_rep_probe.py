"""GPU probe: what short tandem repeats cost stage 1 / count on super-k-mer records, with the windows of period <= 4 counted beside the
records (s1_skm_rep = 1) and without.  The 10 M-read library of bench.py, then the same library with a fraction of its reads replaced
by (AC)n, (AAG)n, (AGAT)n or poly-A reads, by reads of five units at every phase and on both strands in turn (32 table entries in every
workgroup of the make kernel: twice its LDS hash), or with a 40-base (AC) stretch planted inside otherwise unchanged reads — warm-up + 5 steps
each, per-step times (their spread is the yardstick of the comparison with another build), per-kernel clocks, the plan line and a digest
of the outputs.  read2sdbg (stage 1 + stage 2) and count.

    python tools/lowcomplexity_rep_probe.py [--off-only] [--label TEXT] [reads] [planted_fractions] > profiles/r13_lowcomplexity_rep.json
    python tools/lowcomplexity_rep_probe.py --giant --embedded-only [--set NAME=VALUE,...] [--label TEXT] [reads] > one entry of profiles/r16_lowcomplexity_giant.json

--off-only: only the rows with the option off (what a build without the option can run: the parent's half of a comparison).
--giant: the rows with s1_skm_rep = 1 also set s1_skm_giant = 1 (giant bins in slices; a build that does not know the option ignores it:
the parent's half).  --set: further options for those rows (the grid over s1_skm_giant_keys / _work_pct / _max).
--embedded-only: the clean library and the embedded-stretch rows alone — row 7 (1 % of the reads), 9 (0.1 %) and 10 (5 %) — with s1_skm_rep = 1;
--whole-ac: and row 11, 1 % of the reads replaced by (AC)n with s1_skm_rep = 0 and the other options as set (a bin of 1.7 M records)."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from megahit_amd import lib  # noqa: E402

STEPS = 5


def pack(bases):
    """2-bit codes, 16 to a word, MSB first"""
    b = bases.reshape(-1, 16).astype(np.uint32)
    return (b << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def unpack(words):
    return ((words[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).reshape(-1)


def main():
    argv = sys.argv[1:]
    off_only = "--off-only" in argv
    giant, embedded_only, whole_ac = "--giant" in argv, "--embedded-only" in argv, "--whole-ac" in argv
    extra = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in argv[argv.index("--set") + 1].split(",")) if "--set" in argv else {}
    on = dict(extra, s1_skm_giant=1) if giant else dict(extra)  # (what a row with the options on sets beside s1_skm_rep)
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this build"
    pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--label", "--set", "--rows"))]
    n_reads = int(float(pos[0])) if len(pos) > 0 else 10000000
    fracs = [float(x) for x in pos[1].split(",")] if len(pos) > 1 else [0.001, 0.01, 0.05]
    n_reads = n_reads // 16 * 16
    packed = bench.make_reads(n_reads, 0, 1)
    eng = lib.Engine(0)

    def digest(bufs):
        h = hashlib.md5()
        for b, t in bufs:
            h.update(eng.fetch(b, t).tobytes())
        return h.hexdigest()

    def step(engine_name):
        if engine_name == "count":
            eng.count(bench.K, bench.MIN_COUNT)
        else:
            eng.read2sdbg_s1(bench.K, bench.MIN_COUNT)
            plan = eng.last_s1_plan()
            eng.read2sdbg_s2(bench.K, bench.MIN_COUNT)
            return plan
        return eng.last_s1_plan()

    def measure(words, row, what, rep, with_on=None):
        eng.load_sequences(words, n_reads, bench.READ_LEN, None)
        runs = []
        with_on = rep if with_on is None else with_on
        for engine_name in ("read2sdbg", "count"):
            if rep:
                eng.set_option("s1_skm_rep", 1)
            if with_on:
                for name, v in on.items():
                    eng.set_option(name, v)
            try:
                for _ in range(2):
                    plan = step(engine_name)
                eng.synchronize()
                eng.profile(True)
                eng.profile_reset()
                ms = []
                for _ in range(STEPS):
                    t0 = time.perf_counter()
                    step(engine_name)
                    eng.synchronize()
                    ms.append(round((time.perf_counter() - t0) * 1e3, 3))
                st = eng.profile_get()
                eng.profile(False)
            finally:
                if rep:
                    eng.set_option("s1_skm_rep", 0)
                if with_on:  # (back to the defaults of include/mhx.h)
                    for name in on:
                        eng.set_option(name, {"s1_skm_giant_max": 1 << 21, "s1_skm_giant_keys": 4096, "s1_skm_giant_work_pct": 25}.get(name, 0))
            if engine_name == "count":
                d = digest(((lib.BUF_EDGES, np.uint32), (lib.BUF_BUCKET_COUNT, np.uint64), (lib.BUF_MUL_HIST, np.int64), (lib.BUF_FIRST_0_OUT, np.uint32),
                            (lib.BUF_LAST_0_IN, np.uint32)))
            else:
                d = digest(((lib.BUF_SDBG_BYTES, np.uint8), (lib.BUF_BUCKET_COUNT, np.uint64), (lib.BUF_BUCKET_TIPS, np.uint64), (lib.BUF_IS_SOLID, np.uint64),
                            (lib.BUF_MUL_HIST, np.int64)))
            runs.append({"row": row, "library": what, "s1_skm_rep": int(rep), **({"options": on} if with_on and on else {}), "engine": engine_name, "ms_per_step": round(sum(ms) / STEPS, 3), "ms_steps": ms,
                         "spread_ms": round(max(ms) - min(ms), 3), "plan": plan, "digest": d,
                         "kernel_ms_per_step": {k: round(v["ms"] / STEPS, 3) for k, v in sorted(st.items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] / STEPS > 0.3}})
            print("%s | %s | rep %d | %s: %.3f ms (%s)" % (label, what, rep, engine_name, runs[-1]["ms_per_step"], plan[:60]), file=sys.stderr, flush=True)
        return runs

    def replaced(n_plant, unit):
        out = packed.copy()
        out[: n_plant * bench.READ_LEN // 16] = pack(np.tile(np.array(unit, dtype=np.uint8), n_plant * bench.READ_LEN // len(unit) + 1)[: n_plant * bench.READ_LEN])
        return out

    def embedded(n_plant, unit, at, n):
        out = packed.copy()
        b = unpack(out[: n_plant * bench.READ_LEN // 16]).reshape(n_plant, bench.READ_LEN)
        b[:, at:at + n] = np.tile(np.array(unit, dtype=np.uint8), n)[:n]
        out[: n_plant * bench.READ_LEN // 16] = pack(b.reshape(-1))
        return out

    out = {"build": label, "reads": n_reads, "planted_fractions": fracs, "steps": STEPS, "runs": []}
    if embedded_only:
        rows = [int(x) for x in argv[argv.index("--rows") + 1].split(",")] if "--rows" in argv else [2, 9, 7, 10, 11]
        if 2 in rows:
            out["runs"] += measure(packed, 2, "the bench library", True)
        for row, frac in ((9, 0.001), (7, 0.01), (10, 0.05)):
            if row not in rows:
                continue
            n_plant = int(n_reads * frac) // 16 * 16
            out["runs"] += measure(embedded(n_plant, [0, 1], 55, 40), row, "%d reads (%g %%) with a 40-base (AC) stretch at base 55" % (n_plant, frac * 100), True)
        if whole_ac and 11 in rows:
            n_plant = int(n_reads * 0.01) // 16 * 16
            out["runs"] += measure(replaced(n_plant, [0, 1]), 11, "%d reads (1 %%) replaced by (AC)n" % n_plant, False, True)
        print(json.dumps(out, indent=1))
        return
    out["runs"] += measure(packed, 1, "the bench library", False)
    if not off_only:
        out["runs"] += measure(packed, 2, "the bench library", True)
    for frac in fracs:
        n_plant = int(n_reads * frac) // 16 * 16
        words = replaced(n_plant, [0, 1])
        what = "%d reads (%g %%) replaced by (AC)n" % (n_plant, frac * 100)
        out["runs"] += measure(words, 3, what, False)
        if not off_only:
            out["runs"] += measure(words, 4, what, True)
        del words
    n_plant = int(n_reads * 0.01) // 16 * 16
    for name, unit in (("(AAG)n", [0, 0, 2]), ("(AGAT)n", [0, 2, 0, 3])):
        words = replaced(n_plant, unit)
        what = "%d reads (1 %%) replaced by %s" % (n_plant, name)
        out["runs"] += measure(words, 5, what, False)  # (what the same library costs without the option: the other half of row 5's comparison)
        if not off_only:
            out["runs"] += measure(words, 5, what, True)
        del words
    # row 8: five units at every phase and on both strands, read by read in turn — 32 entries meet in every workgroup, twice what its LDS
    # hash holds, so half of them are tallied in the global table window by window
    kinds = []
    for unit in ([0, 1], [0, 0, 2], [0, 2, 0, 3], [0, 0, 0, 1], [0, 1, 2]):
        for ph in range(len(unit)):
            r = np.tile(np.roll(np.array(unit, dtype=np.uint8), ph), bench.READ_LEN)[: bench.READ_LEN]
            kinds += [r, (3 - r[::-1]).astype(np.uint8)]
    mixed = packed.copy()
    mixed[: n_plant * bench.READ_LEN // 16] = pack(np.resize(np.concatenate(kinds), n_plant * bench.READ_LEN))
    for row, words, what in ((6, replaced(n_plant, [0]), "%d reads (1 %%) replaced by poly-A" % n_plant),
                             (7, embedded(n_plant, [0, 1], 55, 40), "%d reads (1 %%) with a 40-base (AC) stretch at base 55" % n_plant),
                             (8, mixed, "%d reads (1 %%) replaced by (AC)n, (AAG)n, (AGAT)n, (AAAC)n, (ACG)n reads in turn, every phase, both strands" % n_plant)):
        out["runs"] += measure(words, row, what, False)
        if not off_only:
            out["runs"] += measure(words, row, what, True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
