"""GPU: the multi-GPU drivers (megahit_amd/csrc/comm.hip) at 4 to 12 ranks, ranks as threads on cuda:0 behind the in-process transport.

tests/test_gpu_comm.py stops at three ranks; an eight-GPU job fills slots of the group-by kernels that three ranks never reach: the
super-k-mer exchange reads one source per sender (k_s1_skm, at most kSkmSrcMax = 8), from nine ranks on the ranks decline it together
and take the pre-sorted exchange (k_s1_stream, up to kStreamSrcMax senders), owner ranges are cut at widths that are not powers of
two, and shards differ in shape.  Every case runs the whole job twice on the same buffers and compares the ranks' outputs with the
oracle on the union of the shards, in rank order.  All ranks must report the same route (route(): the plan line without the figures
that belong to one owner — its record count, its bin range, its giant buckets, its longest read)."""
import re

import numpy as np
import pytest

import oracle_binding as ob
from dist_inputs import reads_of, seqs_with_mult
from megahit_amd import lib, synth
from test_gpu_comm import STAGE_COUNT, STAGE_S1, check_sdbg, load_fixed_reads, run_ranks, sdbg_of

pytestmark = pytest.mark.gpu

SKM = dict(s1_skm=2, s1_skm_max_bin=1 << 30, s1_var_min_fill=5)  # the super-k-mer exchange wherever the ranks can take it
R_SKM, R_PRE, R_CLASSIC = "skm", "presorted", "classic"


def route(plan):
    plan = re.sub(r"\([^)]*\)", "()", plan)
    plan = re.sub(r" \[\d+ giant buckets in slices\]", "", plan)
    return re.sub(r" \[reads of several lengths[^\]]*\]", "", plan)


def check_route(plans, want):
    assert len({route(p) for p in plans}) == 1, plans
    p = plans[0]
    if want == R_SKM:
        assert p.startswith("super-k-mers") and "exchanged by bin" in p, p
    elif want == R_PRE:
        assert "pre-sorted exchange" in p and "exchanged by bin" not in p, p
    else:
        assert "pre-sorted exchange" not in p and "exchanged by bin" not in p, p


def shard_loader(shards):
    def load(r, e):
        pkg = ob.Package(shards[r], reverse=True)
        e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())
    return load


def read2sdbg_job(world, k, m, balance, opts, shards, need_mercy=0):
    """both runs on the same buffers; -> the second run's outputs of every rank"""
    def body(r, e, cm):
        cm.setup(balance, k, m)
        cm.read2sdbg(k, m, need_mercy=need_mercy)
        r1, _r2, nm = cm.read2sdbg(k, m, need_mercy=need_mercy)
        return dict(sdbg=sdbg_of(e), hist=e.fetch(lib.BUF_MUL_HIST, np.int64) if m > 1 else None, n_solid=int(r1.n_solid), plan=e.last_s1_plan(),
                    n_items=int(r1.n_items), sent=cm.bytes_sent(), nm=nm)

    return run_ranks(world, shard_loader(shards), body, opts)


def check_read2sdbg(outs, shards, k, m):
    pkg = ob.Package(sum(shards, []), reverse=True)
    if m > 1:
        s1 = ob.s1(pkg, k, m)
        assert np.array_equal(sum(o["hist"] for o in outs), s1["hist"])
        assert sum(o["n_solid"] for o in outs) == int(sum(bin(int(x)).count("1") for x in s1["is_solid"]))
        assert sum(o["n_items"] for o in outs) == s1["n_items"]
        want = ob.s2(pkg, k, m, s1["is_solid"])
    else:
        s1, want = None, ob.s2(pkg, k, 1, None)
    check_sdbg([o["sdbg"] for o in outs], want)
    return s1, want


def count_job(world, k, m, balance, opts, load):
    def body(r, e, cm):
        cm.setup(balance, k, m)
        cm.count(k, m)
        res = cm.count(k, m)
        return dict(edges=e.fetch(lib.BUF_EDGES, np.uint32), bc=e.fetch(lib.BUF_BUCKET_COUNT, np.uint64), hist=e.fetch(lib.BUF_MUL_HIST, np.int64),
                    first=e.fetch(lib.BUF_FIRST_0_OUT, np.uint32), last=e.fetch(lib.BUF_LAST_0_IN, np.uint32), plan=e.last_s1_plan(), n_items=int(res.n_items))

    return run_ranks(world, load, body, opts)


def check_count(outs, pkg, k, m):
    want = ob.count(pkg, k, m)
    assert np.array_equal(np.concatenate([o["edges"] for o in outs]).reshape(-1, want["wpe"]), want["edges"])
    assert np.array_equal(sum(o["bc"] for o in outs), want["bucket_count"])
    assert np.array_equal(sum(o["hist"] for o in outs), want["hist"])
    assert np.array_equal(np.concatenate([o["first"] for o in outs]), want["first_0_out"])
    assert np.array_equal(np.concatenate([o["last"] for o in outs]), want["last_0_in"])
    assert sum(o["n_items"] for o in outs) == want["n_items"]
    for a in range(len(outs)):  # every bucket has exactly one owner
        for b in range(a + 1, len(outs)):
            assert not np.any((outs[a]["bc"] > 0) & (outs[b]["bc"] > 0))


def pe_shards(world):
    return [reads_of(100 + r, n_pairs=600) for r in range(world)]


@pytest.mark.parametrize("world,k,m,balance,opts", [
    (4, 21, 2, 0, {}), (5, 22, 2, STAGE_S1, {}), (8, 21, 2, 0, {}), (8, 19, 2, STAGE_S1, {}),
    (4, 21, 2, STAGE_S1, {"s1_skm_tags": 1}), (8, 22, 2, 0, {"s1_skm_tags": 1}),
    (5, 21, 2, 0, {"s1_skm_bin_bits": 8}), (8, 21, 2, STAGE_S1, {"s1_skm_bin_bits": 18}),
    (5, 22, 2, STAGE_S1, {"s1_skm_bin_bits": 20}), (8, 21, 2, 0, {"s1_skm_bin_bits": 20}),  # 20 bin bits: a third sort pass
    (4, 19, 2, 0, {"s1_stream_fill": 3}), (8, 21, 2, STAGE_S1, {"s1_stream_fill": 3}),
    (5, 21, 2, 0, {"s1_skm_deal": 0}), (8, 22, 2, 0, {"s1_skm_deal": 0}),
    (4, 21, 1, 0, {}), (8, 21, 1, STAGE_S1, {}),                                          # m = 1: no stage 1, stage 2 at the width
])
def test_read2sdbg_on_the_super_kmer_exchange(world, k, m, balance, opts):
    """up to eight senders per bin, every slot of k_s1_skm's source arrays and LDS bounds in use at world 8"""
    shards = pe_shards(world)
    outs = read2sdbg_job(world, k, m, balance, dict(SKM, **opts), shards)
    s1, _ = check_read2sdbg(outs, shards, k, m)
    if m > 1:
        check_route([o["plan"] for o in outs], R_SKM)
        if world == 8:  # the two runs' records, marks and stage-2 items: under 8 bytes per stage-1 item each (test_gpu_skm.py)
            assert sum(o["sent"] for o in outs) <= 2 * 8 * s1["n_items"], (sum(o["sent"] for o in outs), s1["n_items"])


@pytest.mark.parametrize("world,k,m,balance,opts,want", [
    (9, 21, 2, 0, {}, R_PRE), (12, 22, 2, STAGE_S1, {}, R_PRE), (12, 19, 2, 0, {"s1_skm_tags": 1}, R_PRE),
    (9, 23, 2, STAGE_S1, {}, R_PRE), (12, 27, 2, 0, {}, R_PRE), (9, 29, 2, 0, {}, R_PRE),   # 64-bit table keys
    (12, 31, 2, STAGE_S1, {}, R_CLASSIC), (9, 31, 3, 0, {}, R_CLASSIC),                     # 16-byte records: owner multisplit, sort at the owner
    (9, 21, 2, 0, {"s1_giant_min": 64}, R_PRE), (12, 21, 2, STAGE_S1, {"s1_giant_min": 64}, R_PRE),  # giant buckets: slices cut per sender
    (12, 21, 2, 0, {"s1_stream_fill": 2}, R_PRE),                                          # every bucket overflows its table and splits
    (9, 21, 2, STAGE_S1, {"dist_max_items": 40000}, R_PRE), (12, 22, 2, 0, {"dist_max_items": 40000}, R_PRE),  # bucket-range passes
    (12, 21, 1, 0, {}, None),
])
def test_read2sdbg_beyond_eight_ranks(world, k, m, balance, opts, want):
    """more ranks than k_s1_skm has sources: every rank declines the super-k-mer exchange (s1_skm_dist_applies) and the same libraries
    take the pre-sorted exchange, whose group-by reads a bucket from 9 or 12 senders"""
    shards = pe_shards(world)
    outs = read2sdbg_job(world, k, m, balance, dict(SKM, **opts), shards)
    check_read2sdbg(outs, shards, k, m)
    if want:
        check_route([o["plan"] for o in outs], want)


@pytest.mark.parametrize("bits", [9, 12, 15])
@pytest.mark.parametrize("world", [3, 5, 8])
def test_narrow_stream_prefix_on_several_ranks(world, bits):
    """s1_stream_bits below 16: the owners' slices of the pre-sorted records are cut at lv1 bucket bounds (k_bucket_bounds over 16 bits),
    which the records follow only when they are sorted on at least 16 prefix bits — on several ranks the plan widens the prefix to 16
    (s1.hip s1_plan).  read2sdbg and count, both partitions, against the oracle"""
    k, m = 21, 2
    balance = STAGE_S1 if (world + bits) % 2 else 0
    shards = pe_shards(world)
    outs = read2sdbg_job(world, k, m, balance, dict(s1_skm=0, s1_stream_bits=bits), shards)
    check_read2sdbg(outs, shards, k, m)
    check_route([o["plan"] for o in outs], R_PRE)
    assert outs[0]["plan"].startswith("stream p16 "), outs[0]["plan"]

    reads = [None] * world

    def load(r, e):
        reads[r] = load_fixed_reads(r, e)

    outs = count_job(world, k, m, STAGE_COUNT if not balance else 0, dict(s1_stream_bits=bits), load)
    check_count(outs, ob.Package(sum(reads, []), reverse=True), k, m)
    check_route([o["plan"] for o in outs], R_PRE)
    assert outs[0]["plan"].startswith("count: stream p16 "), outs[0]["plan"]


@pytest.mark.parametrize("world,k,m,opts,want", [
    (4, 21, 2, {}, R_PRE), (5, 22, 1, {}, R_PRE), (8, 23, 3, {}, R_PRE), (12, 27, 15, {}, R_PRE), (12, 21, 2, {}, R_PRE),
    (8, 21, 2, {"s1_giant_min": 64}, R_PRE), (5, 27, 2, {"s1_giant_min": 64}, R_PRE),          # giant buckets: slices cut per sender
    (8, 21, 2, {"dist_max_items": 30000}, R_PRE), (12, 22, 3, {"dist_max_items": 30000}, R_PRE),  # bucket-range passes
    (5, 21, 16, {}, R_CLASSIC), (8, 21, 16, {}, R_CLASSIC),                                      # m = 16: the classic exchange
])
def test_count_on_the_presorted_exchange_wide(world, k, m, opts, want):
    """count: up to twelve senders per bucket into k_s1_stream<COUNT>; the first_0_out / last_0_in events routed back to the read owners"""
    reads = [None] * world

    def load(r, e):
        reads[r] = load_fixed_reads(r, e)

    outs = count_job(world, k, m, STAGE_COUNT if world % 2 else 0, opts, load)
    check_count(outs, ob.Package(sum(reads, []), reverse=True), k, m)
    check_route([o["plan"] for o in outs], want)


@pytest.mark.parametrize("world,k,m,mercy", [(4, 21, 2, 1), (8, 21, 2, 2), (8, 27, 3, 1)])
def test_read2sdbg_mercy_wide(world, k, m, mercy):
    shards = pe_shards(world)
    outs = read2sdbg_job(world, k, m, 0, None, shards, need_mercy=mercy)
    pkg = ob.Package(sum(shards, []), reverse=True)
    s1 = ob.s1(pkg, k, m, tie_stable=mercy == 1)
    n_want, solid = ob.s2_add_mercy(pkg, k, s1["is_solid"], s1["mercy"])
    assert sum(o["nm"] for o in outs) == n_want and n_want > 0
    check_sdbg([o["sdbg"] for o in outs], ob.s2(pkg, k, m, solid))


def long_seqs_with_mult(seed):
    """contig-like sequences, many long enough for k = 61"""
    rng = np.random.default_rng(seed)
    genome = np.random.default_rng(17).integers(0, 4, size=6000, dtype=np.uint8)
    seqs, mult = [], []
    for _ in range(200):
        L = int(rng.integers(30, 240))
        o = int(rng.integers(0, genome.size - L))
        seqs.append(genome[o:o + L].copy())
        mult.append(int(rng.integers(1, 400)))
    return seqs, np.array(mult, dtype=np.uint16)


@pytest.mark.parametrize("world,k", [(4, 39), (8, 39), (4, 61), (8, 61)])
def test_seq2sdbg_wide(world, k):
    gen = seqs_with_mult if k < 60 else long_seqs_with_mult
    inputs = [gen(50 + r) for r in range(world)]

    def load(r, e):
        pkg = ob.Package(inputs[r][0], reverse=False)
        e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())
        e.load_multiplicity(inputs[r][1])

    def body(r, e, cm):
        cm.setup(0, k, 0)
        cm.seq2sdbg(k)
        cm.seq2sdbg(k)
        return sdbg_of(e)

    outs = run_ranks(world, load, body)
    want = ob.seq2sdbg(ob.Package(sum((s for s, _ in inputs), []), reverse=False), np.concatenate([m_ for _, m_ in inputs]), k)
    assert want["bytes"].size > 0
    check_sdbg(outs, want)


def differing_shards(k, low_complexity=True, windowless=True):
    """one shape per rank of eight; rank 7 holds a copy of rank 0's reads (keys reach their multiplicity only across ranks)"""
    rng = np.random.default_rng(5)
    genome = np.random.default_rng(23).integers(0, 4, size=5000, dtype=np.uint8)

    def pe(n_pairs, L, seed):
        return [x for x in synth.gen_pe_reads(n_pairs, genome.size, read_len=L, frag=2 * L + 50, err=0.01, seed=seed, genome=genome)]

    s = [pe(300, 100, 1), pe(200, 150, 2), [x[: rng.integers(k - 4, 151)] for x in pe(250, 150, 3)]]
    if windowless:
        s.append([])                                                            # a rank without reads
        s.append([x[: rng.integers(1, k + 1)] for x in pe(150, 100, 4)])        # only reads shorter than k + 1
    else:
        s += [pe(200, 100, 5), pe(150, 120, 6)]
    if low_complexity:
        s.append([np.zeros(100, dtype=np.uint8) if i % 2 else np.full(100, 2, dtype=np.uint8) for i in range(600)])  # poly-A / poly-G
    else:
        s.append(pe(200, 100, 7))
    s.append([np.tile(np.array([0, 1], dtype=np.uint8), 50)[: int(rng.integers(30, 101))] for _ in range(40)])  # (AC)n
    s.append([x.copy() for x in s[0]])
    return s


@pytest.mark.parametrize("variant", ["eight-shapes", "low-complexity", "no-low-complexity"])
def test_shards_that_differ(variant):
    """eight ranks, eight shapes of shard, read2sdbg on the super-k-mer exchange where the ranks can take it, then count.

    A rank without a (k+1)-mer (no reads, or only short ones) vetoes the super-k-mer exchange for every rank (s1_skm_dist_applies: its
    front has nothing to make) — that is the intended behaviour: the ranks take the pre-sorted exchange together, the rank without reads
    owns its bucket range as any other.  With every rank holding windows, a rank of low-complexity reads makes all ranks give the
    super-k-mer records up together and the plan says why; without that rank they stay on the super-k-mer exchange."""
    k, m = 21, 2
    shards = differing_shards(k, low_complexity=variant != "no-low-complexity", windowless=variant == "eight-shapes")
    assert len(shards) == 8
    outs = read2sdbg_job(8, k, m, STAGE_S1, dict(SKM, s1_skm_max_bin=256), shards)
    check_read2sdbg(outs, shards, k, m)
    plans = [o["plan"] for o in outs]
    if variant == "eight-shapes":
        check_route(plans, R_PRE)
        assert "given up" not in plans[0], plans[0]
    elif variant == "low-complexity":
        check_route(plans, R_PRE)
        assert "[super-k-mer records given up: a rank's bin of low-complexity reads]" in plans[0], plans[0]
    else:
        check_route(plans, R_SKM)
    outs = count_job(8, k, m, STAGE_COUNT, None, shard_loader(shards))
    check_count(outs, ob.Package(sum(shards, []), reverse=True), k, m)


def test_owner_with_an_empty_bucket_range():
    """a few reads of one short genome, eight ranks, the balanced partition: fewer occupied buckets than ranks, so some owners' bucket
    ranges hold nothing (the cuts of mhx_dist_setup repeat a bucket)"""
    world, k, m = 8, 21, 2
    genome = np.random.default_rng(31).integers(0, 4, size=k + 1, dtype=np.uint8)  # one (k+1)-mer: six occupied buckets of the SdBG
    shards = [[genome.copy() for _ in range(3)]] + [[genome.copy()] for _ in range(1, world)]
    outs = read2sdbg_job(world, k, m, STAGE_S1, None, shards)
    _s1, want = check_read2sdbg(outs, shards, k, m)
    assert np.count_nonzero(want["bucket_items"]) < world
    assert any(not o["sdbg"][0] and not o["sdbg"][1].any() for o in outs)
