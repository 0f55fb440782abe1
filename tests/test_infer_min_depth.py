"""CPU: mhx_infer_min_depth (include/mhx.h; host code, no device call) against a Python restatement of
sdbg_pruning::InferMinDepth over Histgram<uint16_t> (assembly/sdbg_pruning.cpp:46-58, utils/histgram.h), doubles compared
exactly: on the reference's own histograms of tests/golden/infer_min_depth.json (tools/make_infer_min_depth_golden.py), where
the restatement must also print what the reference logged, on hand-made histograms and on 200 random ones."""
import json
import math
import os

import numpy as np
import pytest

from megahit_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "infer_min_depth.json")) as f:
    GOLDEN = json.load(f)["cases"]
BINS = 65536


def roundf(x):
    """C's roundf: to the nearest integer, halves away from zero, in float (np.round rounds halves to even)"""
    x = np.float32(x)
    a = np.float32(abs(x))
    f = np.float32(math.floor(a))
    r = f + np.float32(1) if a - f >= np.float32(0.5) else f  # (a - f is exact below 2^23)
    return float(-r if x < 0 else r)


def restatement(hist):
    """hist: {value: count} (zero counts do not exist) -> (min depth, converged, FirstLocalMinimum, rounds run)"""
    bins = sorted((v, c) for v, c in hist.items() if c)
    assert bins, "no valid edge"
    # FirstLocalMinimum, smoothing 4
    best, rising = 0, 0
    for i, (_, c) in enumerate(bins):
        if c <= bins[best][1]:
            best, rising = i, 0
        else:
            rising += 1
            if rising >= 4:
                break
    first_min = 0 if bins[best][0] == bins[-1][0] else bins[best][0]
    depth = float(first_min)
    for rnd in range(1, 101):
        threshold = int(roundf(depth)) & 0xFFFF
        bins = [(v, c) for v, c in bins if v >= threshold]  # TrimLow: what went stays away
        size = sum(c for _, c in bins)
        half = int(size * 0.5)  # size_t(size * p)
        median, run = 0, 0
        for v, c in bins:
            run += c
            if run > half:
                median = v
                break
        nxt = math.sqrt(median)
        if abs(depth - nxt) < 1e-2:
            return depth, True, first_min, rnd
        depth = nxt
    return 1.0, False, first_min, 100


def dense(hist):
    a = np.zeros(BINS, dtype=np.uint64)
    for v, c in hist.items():
        a[v] = c
    return a


def both(hist):
    """the C function and the restatement agree exactly; -> the restatement's tuple"""
    want = restatement(hist)
    got = lib.infer_min_depth(dense(hist))
    assert got == (want[0], want[1]), (got, want)
    return want


def test_golden_file_is_well_formed():
    names = [c["name"] for c in GOLDEN]
    assert names == ["A-p2", "A-p1-final-depth0", "B-m1-p2", "A-orchestrator-p3", "A-defaults", "B-lowcov-firstmin0", "A-highcov-fullmul",
                     "E-k63-mercy"]
    by = {c["name"]: c for c in GOLDEN}
    for c in GOLDEN:
        assert len(c["digests"]) == 8 and all(len(d) == 64 for d in c["digests"].values())
        assert c["route"] in ("PRUNE", "BUBBLE")
        vals = [v for v, _ in c["hist"]]
        assert vals == sorted(set(vals)) and all(0 <= v < BINS and n > 0 for v, n in c["hist"])
        assert sum(n for _, n in c["hist"]) <= c["n_items"]
        assert "%.3f" % float(c["log"]["min_depth"]) == c["log"]["min_depth"] and not c["log"]["unconverged"]
        assert ("--min_depth" in c["args"]) == (c["name"] in ("A-p1-final-depth0", "A-orchestrator-p3"))
    assert by["A-defaults"]["args"] == []
    assert by["A-p1-final-depth0"]["args"][-2:] == ["--min_depth", "0"]
    assert by["A-highcov-fullmul"]["n_large"] >= 0.08 * by["A-highcov-fullmul"]["n_items"] and by["A-highcov-fullmul"]["full_mul"] == 1
    assert max(v for v, _ in by["A-highcov-fullmul"]["hist"]) > 254
    assert by["E-k63-mercy"]["k"] == 63 and by["E-k63-mercy"]["mercy"] and by["B-m1-p2"]["m"] == 1
    assert any(float(c["log"]["min_depth"]) != int(float(c["log"]["min_depth"])) for c in GOLDEN)
    assert sum(c["contigs_differ_from_min_depth_m"] for c in GOLDEN) >= 3


@pytest.mark.parametrize("c", GOLDEN, ids=lambda c: c["name"])
def test_reference_histograms(c):
    """the restatement prints what the reference logged on its own histogram, and the C function equals the restatement"""
    hist = {v: n for v, n in c["hist"]}
    depth, converged, first_min, _ = both(hist)
    assert converged and "%.3f" % depth == c["log"]["min_depth"]
    assert (first_min == 0) == (c["name"] == "B-lowcov-firstmin0")


def test_roundf_by_hand():
    assert [roundf(x) for x in (0.0, 0.49, 0.5, 1.5, 2.5, 2.4999, 3.5, 255.5)] == [0, 0, 1, 2, 3, 2, 4, 256]
    assert roundf(math.sqrt(6.25)) == 3 and roundf(math.sqrt(12.25)) == 4  # halves go away from zero, not to even
    assert roundf(0.49999999) == 1  # float(0.49999999) is 0.5: the rounding happens in float


def test_single_bin():
    depth, converged, first_min, rounds = both({7: 10})
    assert (depth, converged, first_min) == (math.sqrt(7), True, 0) and rounds == 2


def test_falling_counts():
    """1000 // v never rises four times in a row before the last value: the first minimum is the largest value, so 0"""
    depth, converged, first_min, rounds = both({v: 1000 // v for v in range(1, 50)})
    assert (depth, converged, first_min, rounds) == (math.sqrt(11), True, 0, 4)


def test_flat_counts():
    """`<=` moves the running minimum on to the last of equal bins"""
    depth, converged, first_min, _ = both({v: 5 for v in range(1, 300)})
    assert converged and first_min == 0


def test_bin_zero_is_a_value():
    depth, converged, first_min, _ = both({0: 3, 1: 9, 2: 10, 3: 11, 4: 12, 5: 40, 9: 50, 30: 7})
    assert converged and first_min == 0  # the minimum found is bin 0, whose value is also what "none" returns
    depth, converged, first_min, _ = both({0: 50, 1: 20, 2: 3, 3: 9, 4: 30, 5: 60, 6: 90, 7: 40, 20: 5})
    assert converged and first_min == 2
    both({0: 1})
    both({0: 4, 65535: 4})


def non_converging():
    """Derived from the restatement on the machine this test was written on, not run through the reference: the thresholds
    climb 16, 18, 19, 20, ... one per round (the median of what is left is the square two above the threshold: 324, 361, 400, ...)
    and never meet the tolerance"""
    h = {v: 2 for v in range(1, 256)}
    h[16] = 1
    for j in range(16, 256):
        h[j * j] = h.get(j * j, 0) + 1
    h[65535] = 243
    return h


def test_no_convergence():
    h = non_converging()
    assert h[256] == 1 and h[255 * 255] == 1 and sum(1 for v in h if v > 255) == 241
    assert restatement(h) == (1.0, False, 16, 100)
    assert lib.infer_min_depth(dense(h)) == (1.0, False)


def test_empty_histogram_is_an_error():
    with pytest.raises(lib.MhxError, match="no valid edge"):
        lib.infer_min_depth(np.zeros(BINS, dtype=np.uint64))


def test_random_sparse_histograms():
    rng = np.random.default_rng(20240)
    seen = set()
    for i in range(200):
        shape = i % 4
        n_bins = int(rng.integers(1, 60))
        if shape == 0:  # a few values anywhere
            vals = rng.choice(BINS, size=n_bins, replace=False)
            cnts = rng.integers(1, 1000, size=n_bins)
        elif shape == 1:  # a coverage-like profile: errors at the low end, a peak
            vals = np.arange(1, n_bins + 1)
            peak = rng.integers(2, n_bins + 2)
            cnts = (2000 / vals + 300 * np.exp(-((vals - peak) ** 2) / 20.0) + rng.integers(0, 5, size=n_bins)).astype(np.int64) + 1
        elif shape == 2:  # dense low values with bin 0, large counts
            vals = np.arange(0, n_bins)
            cnts = rng.integers(1, 2 ** 40, size=n_bins)
        else:  # squares and their neighbours: medians whose roots sit next to a rounding boundary
            roots = rng.integers(1, 255, size=n_bins)
            vals = np.unique(np.concatenate([roots * roots, roots * roots + roots, roots * roots + roots + 1]))
            cnts = rng.integers(1, 50, size=vals.size)
        want = both({int(v): int(c) for v, c in zip(vals, cnts)})
        seen.add((want[1], want[2] == 0))
    assert (True, True) in seen and (True, False) in seen
