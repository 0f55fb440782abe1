"""CPU: the plain-Python model of `local`'s first half (tests/local_model.py) reproduces the numbers the reference logged for
every small case of tests/golden/local_map.json, and mhx_local_insert_size (host code of libmhx.so, no GPU) gives the model's
mean, sd and range on the model's records.  The cases must have teeth: see test_cases_have_teeth."""
import numpy as np
import pytest

import local_cases
import local_model
import local_util as U
from megahit_amd import lib


@pytest.mark.parametrize("i", U.SMALL, ids=U.case_id)
def test_model_reproduces_reference_log(i):
    c, m, inp = U.CASES[i], U.model(i), U.inputs(i)
    ref = c["ref"]
    assert len(inp["kept"]) == ref["n_contigs"]
    assert m["index_size"] == ref["index_size"]
    assert m["slots"] == c["seed_slots"]
    assert len(ref["libs"]) == len(inp["table"])
    for l, ((b, e, mx, paired), want) in enumerate(zip(inp["table"], ref["libs"])):
        assert want["total"] == e - b
        assert m["aligned"][l] == want["aligned"], "library %d" % l
        assert m["added"][l] == want["added"], "library %d" % l
        if paired:
            assert U.same_printed(m["sizes"][l][0], want["mean"]) and U.same_printed(m["sizes"][l][1], want["sd"]), (m["sizes"][l], want)
        else:
            assert "mean" not in want
    max_len = int(inp["read_len"].max())
    assert (max(s[2] for s in m["sizes"]) // max_len if max_len else 1) == ref["min_reads"]


@pytest.mark.parametrize("i", U.SMALL, ids=U.case_id)
def test_insert_size_of_library_matches_model(i):
    m, inp = U.model(i), U.inputs(i)
    rec = U.records_array(m["recs"], lib.LOCAL_RECORD_DTYPE)
    for (b, e, mx, paired), want in zip(inp["table"], m["sizes"]):
        mean, sd, rng = lib.local_insert_size(rec, inp["read_len"], b, e, mx, paired)
        assert mean == want[0] and rng == want[2]
        assert sd == want[1] or (np.isnan(sd) and np.isnan(want[1]))


def test_insert_size_stops_at_a_full_histogram():
    """2^18 values after two batches of 2^18 reads: the pairs behind them (another fragment length) are not looked at; one pair fewer
    in the first batches and the third batch is read"""
    n = (1 << 19) + 8000
    rec = np.zeros(n, dtype=lib.LOCAL_RECORD_DTYPE)
    rec["valid"] = 1
    rec["query_to"] = 59
    rec["strand"][1::2] = 1
    rec["contig_from"][0::2] = 1000
    rec["contig_to"][0::2] = 1059
    rec["contig_from"][1::2] = 1140
    rec["contig_to"][1::2] = 1199
    rec["contig_from"][(1 << 19) + 1::2] += 100
    rec["contig_to"][(1 << 19) + 1::2] += 100
    lens = np.full(n, 60, dtype=np.uint32)
    assert lib.local_insert_size(rec, lens, 0, n, 60, True) == (200.0, 0.0, 200)
    rec["valid"][10] = 0
    mean, sd, rng = lib.local_insert_size(rec, lens, 0, n, 60, True)
    assert mean == 201.0 and sd > 0  # 2^18 - 1 values of 200 and 4000 of 300 (too many for the trim of half a per cent)
    assert lib.local_insert_size(rec, lens, 0, n, 60, False) == (0.0, 0.0, 59)


def test_cases_have_teeth():
    """over the committed cases the reference itself logs: a library with aligned < total, a paired library whose range is not
    max_read_len - 1, an index smaller than its seed slots; and (from the model, whose counts equal the reference's) items at a
    contig's start and at a contig's end"""
    unaligned = rng_differs = dup = False
    for c in U.CASES:
        dup |= c["ref"]["index_size"] < c["seed_slots"]
        for want in c["ref"]["libs"]:
            unaligned |= want["aligned"] < want["total"]
    for i in range(len(U.CASES)):
        for (b, e, mx, paired), want in zip(U.inputs(i)["table"], U.CASES[i]["ref"]["libs"]):
            if paired and "nan" not in want["sd"]:
                mean, sd = float(want["mean"]), float(want["sd"])
                rng_differs |= mean >= mx and min(650, int(min(2 * mean, mean + 3 * sd))) != mx - 1
    assert unaligned and rng_differs and dup
    at_start = at_end = False
    for i in U.SMALL:
        off = U.model(i)["offsets"]
        if U.model(i)["added"] != [l["added"] for l in U.CASES[i]["ref"]["libs"]]:
            continue
        sizes = [off[g + 1] - off[g] for g in range(len(off) - 1)]
        at_start |= any(sizes[0::2])
        at_end |= any(sizes[1::2])
    assert at_start and at_end


def test_cases_reach_the_branches():
    """over the small cases the model's records hold: both strands, clipped records at either side, 15 and more mismatches, reads too
    short to map, a read of mappable length left invalid where two contigs fit equally well, mates' items and singles' items"""
    seen = set()
    for i in U.SMALL:
        m, inp = U.model(i), U.inputs(i)
        for r, n in zip(m["recs"], inp["read_len"]):
            if not r["valid"]:
                seen.add("short" if n < 50 else "invalid")
                continue
            seen.add("strand%d" % r["strand"])
            if r["query_from"] > 0:
                seen.add("clipped_left")
            if r["query_to"] < n - 1:
                seen.add("clipped_right")
            if r["mismatch"] >= 15:
                seen.add("mismatch15")
        for v in m["items"]:
            seen.add("mate_item" if (v >> 49) & 1 else "single_item")
        if U.CASES[i]["name"] == "rc_ends" and U.CASES[i]["sparsity"] == 8:
            # reads 0..119 come from the stretch of contig 0 whose reverse complement ends contig 1: some lie inside it wholly
            assert any(not r["valid"] for r in m["recs"][:120]) and any(r["valid"] for r in m["recs"][:120])
    assert seen >= {"short", "invalid", "strand0", "strand1", "clipped_left", "clipped_right", "mismatch15", "mate_item", "single_item"}, seen


def test_seed32_cases_hold_the_keys_that_use_all_64_bits():
    """at 32 bases a key fills the 64-bit word: the cases hold key 0 (a run of 32 T; used in `seed32`, flagged in `seed32_dup`), keys with
    bit 63 set, and a window equal to its own reverse complement; reads reach the index through key 0"""
    seen = set()
    for i in U.SMALL:
        c = U.CASES[i]
        if c["seed_kmer"] != 32:
            continue
        kept = U.inputs(i)["kept"]
        index, _ = local_model.build_index(kept, 32, c["sparsity"])
        assert 0 in index and any(k >> 63 for k in index)
        assert (index[0] is local_model.DUP) == (c["name"] == "seed32_dup")
        seen.add(c["name"])
        own = next(local_model._windows(kept[0][800:832], 32))
        assert index[own[1]] == (0, 800, 0)
        reads = local_cases.all_reads(U.inputs(i)["libs"])
        assert any(key == 0 for r in reads for _, key, _ in local_model._windows(r, 32))
    assert seen == {"seed32", "seed32_dup"}
