"""Randomised libraries on 2-9 thread ranks through mhx_dist_read2sdbg with the super-k-mer exchange, against the oracle on the union (GPU).
Every third job or so is a `count` instead (mhx_dist_count with count_skm_dist = 1: worlds 2-8, k 19-21, min count 1-2, the same knobs).

    python tools/fuzz_skm_dist.py [seconds] [seed]

Sometimes one rank's shard is empty or degenerate (reads shorter than k + 1, a single homopolymer read): such a rank vetoes the
super-k-mer exchange of read2sdbg for every rank, as do nine ranks (more senders than k_s1_skm takes); the job then runs on the pre-sorted
exchange.  `count` keeps the route with ranks that hold no window; a lone homopolymer read makes its ranks give up together."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_binding as ob  # noqa: E402
from megahit_amd import lib  # noqa: E402
from fuzz_skm import library  # noqa: E402
from test_gpu_comm import run_ranks, sdbg_of, check_sdbg  # noqa: E402
from test_gpu_wide_worlds import check_count, count_job, shard_loader  # noqa: E402


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    t0, rounds, on_path = time.time(), 0, 0
    while time.time() - t0 < seconds:
        seed = seed0 + rounds
        rng = np.random.default_rng(seed)
        world = int(rng.integers(2, 10))
        k = int(rng.integers(19, 23))
        crng = np.random.default_rng([seed, 7])  # (a stream of its own: a seed's read2sdbg job is what it was before `count` jobs were drawn)
        counting = crng.random() < 0.35
        if counting:
            world, k = int(crng.integers(2, 9)), int(crng.integers(19, 22))
        shards = [library(np.random.default_rng(seed * 10 + r)) for r in range(world)]
        odd = ""
        if rng.random() < 0.25:  # one empty or degenerate shard
            r_odd, odd = int(rng.integers(0, world)), str(rng.choice(["empty", "short", "homopolymer"]))
            shards[r_odd] = {"empty": [], "short": [x[: int(rng.integers(0, k + 1))] for x in shards[r_odd][:50]],
                             "homopolymer": [np.zeros(int(rng.integers(k + 1, 200)), dtype=np.uint8)]}[odd]
        opts = dict(s1_skm=2, s1_var_min_fill=1, s1_skm_max_bin=1 << 30, s1_skm_cap_pct=400)
        if rng.random() < 0.5:
            opts["s1_skm_bin_bits"] = int(rng.choice([8, 9, 12, 16, 18, 20]))
        if rng.random() < 0.5:
            opts["s1_stream_fill"] = int(rng.choice([3, 17, 200, 4000]))
        if rng.random() < 0.3:
            opts["s1_skm_tags"] = 1
        if rng.random() < 0.3:
            opts["s1_skm_deal"] = int(rng.integers(0, 2))  # (2 is the default)
        if rng.random() < 0.15:
            opts["s1_skm_max_bin"] = int(rng.choice([8, 500]))
        if rng.random() < 0.3:
            opts["s1_skm_split"] = 0
        if rng.random() < 0.3:
            opts["s1_skm_split_stage"] = int(rng.choice([0, 64, 700]))
        if rng.random() < 0.4:
            opts["s1_skm_make_grid"] = int(rng.choice([1, 2, 5]))

        if counting:
            m = int(crng.integers(1, 3))
            opts["count_skm_dist"] = 1
            if crng.random() < 0.3:
                opts["count_skm_group"] = 4
            outs = count_job(world, k, m, 3 * int(seed % 2), opts, shard_loader(shards))
            try:
                check_count(outs, ob.Package(sum(shards, []), reverse=True), k, m)
            except AssertionError as ex:
                print("seed %d: count, world %d k %d m %d %s *** %s | %s" % (seed, world, k, m, opts, ex, outs[0]["plan"]), flush=True)
                sys.exit(1)
            on_path += outs[0]["plan"].startswith("count: super-k-mers")
            print("seed %d: count, world %d%s, %d reads, k %d, m %d, %s | %s" % (seed, world, " (%s shard)" % odd if odd else "", sum(len(s) for s in shards), k, m,
                                                                                 " ".join("%s=%d" % kv for kv in sorted(opts.items()) if kv[0] not in ("s1_skm", "s1_var_min_fill", "s1_skm_cap_pct")),
                                                                                 outs[0]["plan"][:47]), flush=True)
            rounds += 1
            continue

        def load(r, e):
            pkg = ob.Package(shards[r], reverse=True)
            e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())

        def body(r, e, cm):
            cm.setup(int(seed % 2), k, 2)
            r1, r2, _ = cm.read2sdbg(k, 2)
            return sdbg_of(e) + (e.fetch(lib.BUF_MUL_HIST, np.int64), int(r1.n_solid), e.last_s1_plan(), int(r1.n_items))

        outs = run_ranks(world, load, body, opts)
        pkg = ob.Package(sum(shards, []), reverse=True)
        s1 = ob.s1(pkg, k, 2)
        try:
            assert np.array_equal(sum(o[4] for o in outs), s1["hist"]), "histogram"
            assert sum(o[5] for o in outs) == int(sum(bin(int(x)).count("1") for x in s1["is_solid"])), "n_solid"
            check_sdbg(outs, ob.s2(pkg, k, 2, s1["is_solid"]))
        except AssertionError as ex:
            print("seed %d: world %d k %d %s *** %s | %s" % (seed, world, k, opts, ex, outs[0][6]), flush=True)
            sys.exit(1)
        on_path += outs[0][6].startswith("super-k-mers")
        print("seed %d: world %d%s, %d reads, k %d, %s | %s" % (seed, world, " (%s shard)" % odd if odd else "", sum(len(s) for s in shards), k,
                                                            " ".join("%s=%d" % kv for kv in sorted(opts.items()) if kv[0] not in ("s1_skm", "s1_var_min_fill", "s1_skm_cap_pct")), outs[0][6][:40]), flush=True)
        rounds += 1
    print("%d rounds, %d on the super-k-mer exchange, all equal to the oracle" % (rounds, on_path))


if __name__ == "__main__":
    main()
