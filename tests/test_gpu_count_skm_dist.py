"""GPU: `count` on super-k-mer records across several ranks (comm.hip dist_count_skm; opt-in, option count_skm_dist).

Every rank makes the 16-byte records of its reads (k_skm_make<.., COUNT> under the global layout), the records cross by minimizer bin, the
bin owners group the windows (k_count_skm<.., EVENTS>: the windows of flagged keys leave as events), the solid edges cross once more to the
owners of their lv1 buckets, the events go to the ranks that hold the reads, and the homopolymer tallies are summed over the ranks.  Ranks
are threads on cuda:0 behind the in-process transport; every case runs the job twice on the same buffers and compares the ranks' outputs
with the oracle's single KmerCounter run on the union of the shards (check_count: edges, bucket counts, histogram, first_0_out, last_0_in,
n_items, one owner per bucket)."""
import numpy as np
import pytest

import oracle_binding as ob
from dist_inputs import reads_of
from megahit_amd import lib, synth
from test_gpu_comm import STAGE_COUNT, load_fixed_reads, run_ranks
from test_gpu_wide_worlds import check_count, count_job, route, shard_loader

pytestmark = pytest.mark.gpu

SKM = dict(s1_skm=2, s1_skm_max_bin=1 << 30, s1_var_min_fill=5, count_skm_dist=1)


def check_taken(plans):
    assert len({route(p) for p in plans}) == 1, plans
    for p in plans:
        assert p.startswith("count: super-k-mers") and "exchanged by bin" in p, p


def check_declined(plans, why=None):
    assert len({route(p) for p in plans}) == 1, plans
    for p in plans:
        assert "pre-sorted exchange" in p and "exchanged by bin" not in p, p
        if why:
            assert "[super-k-mer records given up: %s]" % why in p, p
        else:
            assert "given up" not in p, p


def fixed_job(world, k, m, balance, opts):
    """the fixed-length shards of test_gpu_comm.py: rank 1 holds 40 poly-A reads — homopolymer windows on one rank only, which reach the
    histogram and the edges through the sum over the ranks"""
    reads = [None] * world

    def load(r, e):
        reads[r] = load_fixed_reads(r, e)

    outs = count_job(world, k, m, balance, opts, load)
    check_count(outs, ob.Package(sum(reads, []), reverse=True), k, m)
    return outs


def shard_job(shards, k, m, balance, opts):
    outs = count_job(len(shards), k, m, balance, opts, shard_loader(shards))
    check_count(outs, ob.Package(sum(shards, []), reverse=True), k, m)
    return outs


@pytest.mark.parametrize("world,k,m,balance", [
    (2, 21, 2, 0), (2, 19, 1, STAGE_COUNT), (3, 20, 2, STAGE_COUNT), (4, 21, 1, 0), (4, 20, 2, STAGE_COUNT), (5, 19, 2, STAGE_COUNT),
    (8, 21, 2, STAGE_COUNT), (8, 20, 1, 0),
])
def test_route_taken(world, k, m, balance):
    """the ranks agree on the route and say so; with the balanced partition the edges' owner ranges are not uniform"""
    outs = fixed_job(world, k, m, balance, SKM)
    check_taken([o["plan"] for o in outs])


@pytest.mark.parametrize("world,bits", [(8, 8), (8, 18), (4, 20)])
def test_every_source_slot_of_a_bin(world, bits):
    """256 bins: every bin is fed by all eight senders (every slot of k_count_skm's source arrays and LDS bounds); 18 and 20 bin bits: a
    third sort pass before the exchange"""
    outs = fixed_job(world, 21, 2, 0, dict(SKM, s1_skm_bin_bits=bits))
    check_taken([o["plan"] for o in outs])
    assert "2^%d bins" % bits in outs[0]["plan"], outs[0]["plan"]


@pytest.mark.parametrize("world,opts", [
    (4, {"s1_skm_tags": 1}), (8, {"s1_skm_tags": 1}), (8, {"count_skm_group": 4}), (4, {"count_skm_group": 4, "s1_skm_tags": 1}),
    (4, {"s1_skm_split": 0}), (8, {"s1_skm_split": 0}), (4, {"s1_stream_fill": 3}), (8, {"s1_stream_fill": 3}),
], ids=lambda v: ",".join("%s=%d" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_kernel_variants(world, opts):
    """the four instantiations of k_count_skm<.., EVENTS> (position tags, four chunks per round), records made without the split, and tables
    that overflow and run in rounds (the second expansion then looks only at the keys of its round)"""
    outs = fixed_job(world, 21, 2, STAGE_COUNT if world == 8 else 0, dict(SKM, **opts))
    check_taken([o["plan"] for o in outs])


@pytest.mark.parametrize("world,k,m", [(3, 21, 2), (8, 19, 1), (4, 20, 2)])
def test_reads_of_several_lengths(world, k, m):
    """ragged shards, 10 to 100 bases: every read takes the blocks of the longest, reads without a window make nothing"""
    outs = shard_job([reads_of(100 + r, n_pairs=600) for r in range(world)], k, m, STAGE_COUNT, SKM)
    check_taken([o["plan"] for o in outs])


def genome_reads(seed, n_pairs=300):
    genome = np.random.default_rng(77).integers(0, 4, size=3000, dtype=np.uint8)
    return [x for x in synth.gen_pe_reads(n_pairs, genome.size, read_len=100, frag=250, err=0.01, seed=seed, genome=genome)]


def edge_present(want, key64):
    e = want["edges"]
    return bool(np.any((e[:, 0] == np.uint32(key64 >> 32)) & ((e[:, 1] & np.uint32(0xFFFF0000)) == np.uint32(key64 & 0xFFFF0000))))


def test_homopolymer_key_solid_only_in_the_sum():
    """one poly-C window of k + 1 bases (A in front, G behind) on each of two ranks, none elsewhere, m = 2: neither rank sees a solid key,
    the sum does — it must be an edge and in the histogram"""
    world, k, m = 4, 21, 2
    rng = np.random.default_rng(8)
    shards = [genome_reads(400 + r) for r in range(world)]
    for r in (0, 2):
        read = np.concatenate([rng.integers(0, 4, size=39, dtype=np.uint8), [0], np.full(k + 1, 1, dtype=np.uint8), [2],
                               rng.integers(0, 4, size=100 - 39 - 2 - (k + 1), dtype=np.uint8)]).astype(np.uint8)
        assert read.size == 100
        shards[r].insert(5 + r, read)
    pkg = ob.Package(sum(shards, []), reverse=True)
    want = ob.count(pkg, k, m)
    key = 0x5555555555555555 & (~0 << (64 - 2 * (k + 1))) & 0xFFFFFFFFFFFFFFFF
    assert edge_present(want, key)  # (the shards are what the case says they are)
    outs = shard_job(shards, k, m, 0, SKM)
    check_taken([o["plan"] for o in outs])
    got = np.concatenate([o["edges"] for o in outs]).reshape(-1, 2)
    assert edge_present({"edges": got}, key)
    # without either of the two reads the key is not solid: the oracle agrees that it takes both ranks
    lone = [s if r != 2 else [x for x in s if not np.array_equal(x[40:40 + k + 1], np.full(k + 1, 1))] for r, s in enumerate(shards)]
    assert not edge_present(ob.count(ob.Package(sum(lone, []), reverse=True), k, m), key)


def test_flagged_homopolymer_key_gives_up_on_every_rank():
    """two ranks each hold one read that is exactly k + 1 A's: solid in the sum, nothing in front or behind — its windows would move
    first_0_out / last_0_in, which the tallies cannot do: every rank knows after the all-reduce and all take the pre-sorted exchange"""
    world, k, m = 4, 21, 2
    shards = [genome_reads(500 + r) for r in range(world)]
    for r in (1, 3):
        shards[r].insert(7, np.zeros(k + 1, dtype=np.uint8))
    outs = shard_job(shards, k, m, STAGE_COUNT, SKM)
    check_declined([o["plan"] for o in outs], "a solid homopolymer key without an in- or out-edge")


@pytest.mark.parametrize("kind", ["three-empty", "one-windowless"])
def test_ranks_without_work(kind):
    """a rank without a window sends no records, owns its bins and its lv1 buckets, and takes part in every collective"""
    world, k, m = 8, 21, 2
    shards = [genome_reads(600 + r, n_pairs=250) for r in range(world)]
    if kind == "three-empty":
        for r in (0, 4, 7):
            shards[r] = []
    else:
        rng = np.random.default_rng(3)
        shards[5] = [x[: rng.integers(1, k + 1)] for x in shards[5]]
    outs = shard_job(shards, k, m, STAGE_COUNT if kind == "three-empty" else 0, SKM)
    check_taken([o["plan"] for o in outs])


def test_forced_give_up_and_recovery():
    """an event region of one entry overflows at some owner: all ranks give up together, the pre-sorted exchange redoes the pass from clean
    arrays; with the cap lifted the same handles take the route again"""
    world, k, m = 3, 21, 2
    reads = [None] * world

    def load(r, e):
        reads[r] = load_fixed_reads(r, e)

    def fetch(e, res):
        return dict(edges=e.fetch(lib.BUF_EDGES, np.uint32), bc=e.fetch(lib.BUF_BUCKET_COUNT, np.uint64), hist=e.fetch(lib.BUF_MUL_HIST, np.int64),
                    first=e.fetch(lib.BUF_FIRST_0_OUT, np.uint32), last=e.fetch(lib.BUF_LAST_0_IN, np.uint32), plan=e.last_s1_plan(), n_items=int(res.n_items))

    def body(r, e, cm):
        cm.setup(STAGE_COUNT, k, m)
        cm.count(k, m)
        capped = fetch(e, cm.count(k, m))
        e.set_option("count_skm_ev_cap", 0)
        return capped, fetch(e, cm.count(k, m))

    outs = run_ranks(world, load, body, dict(SKM, count_skm_ev_cap=1))
    pkg = ob.Package(sum(reads, []), reverse=True)
    check_count([o[0] for o in outs], pkg, k, m)
    check_declined([o[0]["plan"] for o in outs], "an owner's edge or event region overflowed")
    check_count([o[1] for o in outs], pkg, k, m)
    check_taken([o[1]["plan"] for o in outs])


@pytest.mark.parametrize("world,k,m,opts", [
    (9, 21, 2, {}),                          # more ranks than the group-by has sources
    (4, 22, 2, {}), (4, 21, 3, {}),          # k + 10 bases do not fit a record; seen-once / seen-twice bits serve min count <= 2
    (3, 21, 2, {"dist_max_items": 30000}),   # bucket-range passes
])
def test_declines(world, k, m, opts):
    outs = fixed_job(world, k, m, STAGE_COUNT, dict(SKM, **opts))
    check_declined([o["plan"] for o in outs])


def test_knob_off_changes_nothing():
    outs = fixed_job(4, 21, 2, 0, dict(SKM, count_skm_dist=0))
    check_declined([o["plan"] for o in outs])


@pytest.mark.parametrize("world", [4, 8])
def test_bytes_on_the_wire(world):
    """what the ranks hand to each other in one job (records, edges, events) against the pre-sorted exchange of the same shards in the same
    test: 12 bytes per foreign window there; here 16 bytes per record of ~3.5 windows, plus 8 per foreign solid edge and event.
    Measured on these shards (k = 21, m = 2; bytes with the knob set / with it at 0): world 4: 1 122 472 / 2 867 636 = 0.391;
    world 8: 2 669 888 / 6 656 120 = 0.401"""
    k, m = 21, 2
    sums = {}
    for knob in (1, 0):
        reads = [None] * world

        def load(r, e):
            reads[r] = load_fixed_reads(r, e)

        def body(r, e, cm):
            cm.setup(0, k, m)
            cm.count(k, m)
            cm.bytes_sent(reset=True)
            cm.count(k, m)
            return dict(sent=cm.bytes_sent(), plan=e.last_s1_plan())

        outs = run_ranks(world, load, body, dict(SKM, count_skm_dist=knob))
        (check_taken if knob else check_declined)([o["plan"] for o in outs])
        sums[knob] = sum(o["sent"] for o in outs)
    print("bytes sent, world %d: exchanged by bin %d, pre-sorted exchange %d, ratio %.3f" % (world, sums[1], sums[0], sums[1] / sums[0]))
    assert sums[1] < sums[0], sums
