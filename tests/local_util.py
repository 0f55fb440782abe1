"""Shared by the `local` mapping tests: the golden cases and, per case, the model's results (computed once)."""
import functools
import json
import math
import os

import numpy as np

import local_cases
import local_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_map.json")
with open(GOLDEN) as f:
    CASES = json.load(f)
SMALL = [i for i, c in enumerate(CASES) if c["name"] not in local_cases.LARGE]
LARGE = [i for i, c in enumerate(CASES) if c["name"] in local_cases.LARGE]


def case_id(i):
    c = CASES[i]
    return "%s-k%d-s%d" % (c["name"], c["seed_kmer"], c["sparsity"])


def printed(x):
    """a double as the reference's log prints it ({.2}: two decimals); the sign of a NaN is not compared"""
    return "nan" if math.isnan(x) else "%.2f" % x


def same_printed(x, golden_text):
    return printed(x) == golden_text.lstrip("-") if "nan" in golden_text else printed(x) == golden_text


@functools.lru_cache(maxsize=None)
def inputs(i):
    """-> dict(kept contigs, libraries, read lengths, library table) of case i"""
    contigs, libs = local_cases.build(CASES[i])
    return dict(kept=local_model.keep_contigs(contigs, local_cases.MIN_CONTIG_LEN), libs=libs, read_len=local_cases.read_lengths(libs),
                table=local_cases.lib_table(libs))


@functools.lru_cache(maxsize=None)
def model(i):
    """-> dict(index_size, slots, recs, sizes [(mean, sd, range)], aligned, added, items, offsets) of small case i"""
    c, inp = CASES[i], inputs(i)
    index, slots = local_model.build_index(inp["kept"], c["seed_kmer"], c["sparsity"])
    reads = local_cases.all_reads(inp["libs"])
    recs = local_model.map_reads(reads, index, inp["kept"], c["seed_kmer"], c["min_mapping_len"], c["similarity"])
    read_len = [int(x) for x in inp["read_len"]]
    sizes = [local_model.insert_size(recs, read_len, b, e, mx, p) for b, e, mx, p in inp["table"]]
    libs = [(b, e, p, s[2]) for (b, e, mx, p), s in zip(inp["table"], sizes)]
    aligned, added, items, offsets = local_model.collect(recs, read_len, inp["kept"], libs)
    return dict(index_size=len(index), slots=slots, recs=recs, sizes=sizes, aligned=aligned, added=added, items=items, offsets=offsets)


def records_array(recs, dtype):
    out = np.zeros(len(recs), dtype=dtype)
    for name in dtype.names:
        out[name] = [r[name] for r in recs]
    return out
