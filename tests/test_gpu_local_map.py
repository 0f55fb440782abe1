"""GPU: mhx_local_index / _map / _collect against the plain-Python model (tests/local_model.py) record by record and item by item,
and against the numbers the reference logged (tests/golden/local_map.json), on the cases of tests/local_cases.py: read lengths
49 .. 151 and reads shorter than the seed, 0 / 3 / 18 / 25 % errors, reads hanging over contig ends by 1, 74, 75, 76 bases,
contigs of 199 and 200 bases and a loop contig, an exact repeat shared by two contigs, reverse-complementary contig ends (ties),
paired and single-end libraries with their own ranges, no contig at all, seeds of 31, 24 and 32 bases (at 32 a key fills the 64-bit word:
a run of 32 T whose key is 0, used and flagged, keys with bit 63 set, a self-complementary window), sparsity 1 and 8.  The large
case (two batches of the insert-size estimate) is compared with the golden numbers only."""
import numpy as np
import pytest

import local_cases
import local_util as U
from megahit_amd import lib

pytestmark = pytest.mark.gpu


def run(engine, i):
    """index + map of case i -> (index size, valid records, records)"""
    c, inp = U.CASES[i], U.inputs(i)
    words, start = local_cases.pack_contigs(inp["kept"])
    engine.load_bin_records(local_cases.bin_records(inp["libs"]), inp["read_len"].size, reverse=False)
    n_keys = engine.local_index(words, len(inp["kept"]), start, c["seed_kmer"], c["sparsity"])
    n_valid = engine.local_map(c["min_mapping_len"], c["similarity"])
    return n_keys, n_valid, engine.local_records()


@pytest.mark.parametrize("i", U.SMALL, ids=U.case_id)
def test_records_and_items_equal_model(engine, i):
    c, inp, m = U.CASES[i], U.inputs(i), U.model(i)
    n_keys, n_valid, rec = run(engine, i)
    assert n_keys == m["index_size"] == c["ref"]["index_size"]
    want = U.records_array(m["recs"], lib.LOCAL_RECORD_DTYPE)
    bad = np.nonzero(rec != want)[0]
    assert bad.size == 0, "read %d: got %s, model %s" % (bad[0], rec[bad[0]], want[bad[0]])
    assert n_valid == int(want["valid"].sum())
    libs = []
    for (b, e, mx, paired), size in zip(inp["table"], m["sizes"]):
        mean, sd, rng = lib.local_insert_size(rec, inp["read_len"], b, e, mx, paired)
        assert (mean, rng) == (size[0], size[2])
        libs.append((b, e, paired, rng))
    aligned, added, items, offsets = engine.local_collect(libs)
    assert [int(x) for x in aligned] == m["aligned"] == [l["aligned"] for l in c["ref"]["libs"]]
    assert [int(x) for x in added] == m["added"] == [l["added"] for l in c["ref"]["libs"]]
    assert np.array_equal(offsets, np.array(m["offsets"], dtype=np.uint64))
    assert np.array_equal(items, np.array(m["items"], dtype=np.uint64))


@pytest.mark.parametrize("i", U.LARGE, ids=U.case_id)
def test_large_case_equals_reference_log(engine, i):
    c, inp = U.CASES[i], U.inputs(i)
    n_keys, n_valid, rec = run(engine, i)
    assert n_keys == c["ref"]["index_size"]
    libs = []
    for (b, e, mx, paired), want in zip(inp["table"], c["ref"]["libs"]):
        mean, sd, rng = lib.local_insert_size(rec, inp["read_len"], b, e, mx, paired)
        assert U.same_printed(mean, want["mean"]) and U.same_printed(sd, want["sd"]), (mean, sd, want)
        libs.append((b, e, paired, rng))
    aligned, added, items, offsets = engine.local_collect(libs)
    assert [int(x) for x in aligned] == [l["aligned"] for l in c["ref"]["libs"]] and n_valid == int(aligned.sum())
    assert [int(x) for x in added] == [l["added"] for l in c["ref"]["libs"]]
    assert max(l[3] for l in libs) // int(inp["read_len"].max()) == c["ref"]["min_reads"]
    assert offsets.size == 2 * len(inp["kept"]) + 1 and offsets[-1] == items.size == int(added.sum())


def test_no_contig_gives_empty_results(engine):
    i = next(j for j in U.SMALL if U.CASES[j]["name"] == "no_contig")
    n_keys, n_valid, rec = run(engine, i)
    assert n_keys == 0 and n_valid == 0 and not rec.view(np.uint32).any()
    aligned, added, items, offsets = engine.local_collect([(b, e, p, 99) for b, e, mx, p in U.inputs(i)["table"]])
    assert not aligned.any() and not added.any() and items.size == 0 and offsets.tolist() == [0]


def test_errors(engine):
    i = U.SMALL[0]
    run(engine, i)
    n = U.inputs(i)["read_len"].size
    with pytest.raises(lib.MhxError, match="2\\^14"):
        engine.local_collect([(0, n, True, (1 << 14) + 1)])
    with pytest.raises(lib.MhxError, match="outside the loaded reads"):
        engine.local_collect([(0, n + 2, True, 300)])
    with pytest.raises(lib.MhxError, match="odd number"):
        engine.local_collect([(0, n - 1, True, 300)])
    with pytest.raises(lib.MhxError, match="seed_kmer"):
        engine.local_index(np.zeros(1, dtype=np.uint32), 0, np.zeros(1, dtype=np.uint64), 33, 8)
    with pytest.raises(lib.MhxError, match="run mhx_local_index first"):  # the failed call dropped the index
        engine.local_map()
    run(engine, i)
    engine.trim()
    with pytest.raises(lib.MhxError, match="run mhx_local_index first"):
        engine.local_map()
    with pytest.raises(lib.MhxError, match="run mhx_local_index first"):
        engine.local_collect([(0, n, True, 300)])


def test_records_go_stale_with_the_reads(engine):
    """another library of as many reads loaded behind mhx_local_map: its records do not belong to those reads"""
    i = U.SMALL[0]
    run(engine, i)
    inp = U.inputs(i)
    n = inp["read_len"].size
    engine.load_bin_records(local_cases.bin_records(inp["libs"]), n, reverse=False)
    with pytest.raises(lib.MhxError, match="run mhx_local_map on the loaded reads first"):
        engine.local_collect([(0, n, True, 300)])
    engine.local_map()
    engine.local_collect([(0, n, True, 300)])
