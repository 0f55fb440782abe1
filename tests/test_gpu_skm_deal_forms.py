"""GPU: every form of the dealing in stage 1's group-by on super-k-mer records (megahit_amd/csrc/s1_skm.hip k_s1_skm, knob s1_skm_deal:
0 every lane expands its own record; 1 the windows of a wavefront's 64 records are dealt to the lanes and a window's record comes over
with six shuffles; 2 with three — the record's lane and the window's index in it come from the bitmap of run heads, the reverse
complement from the window itself: megahit_amd/csrc/skm_deal.h, whose arithmetic tests/host/skm_deal_check.cpp checks on the CPU).
Each case goes through test_gpu_skm.run: is_solid, the multiplicity histogram, the item and solid counts and the SdBG against the oracle.
The settings are those at which the dealing takes another path: rounds redone in halves (the second-hash filter), a probe limit, the
kernel with position tags, and few large bins (many trips per bin, full wavefronts: chunks 1 to 3 run and the carry is read).  The
second group of four chunks needs a wavefront of more than 256 windows, which 64 records of about 3.4 windows hardly ever are: the
library of long_run_reads is made for it, and one test counts that it gets there."""
import re

import numpy as np
import pytest

from test_gpu_round3_knobs import fixed_library
from test_gpu_skm import RESET, run

pytestmark = pytest.mark.gpu

FORMS = [0, 1, 2]  # every form the sources keep
LIBRARIES = [("pe100", 21, 2), ("repeats100", 22, 2), ("short30", 21, 2), ("tiny60", 19, 1), ("pe100", 20, 1)]
SETTINGS = [dict(), dict(s1_stream_fill=40), dict(s1_stream_probes=2), dict(s1_skm_tags=1), dict(s1_skm_bin_bits=11)]


def ids(o):
    return ",".join("%s=%d" % kv for kv in o.items()) or "default"


assert "s1_skm_deal" in RESET  # (run puts the knob back after every case: to 1, the default before form 2)


@pytest.fixture(autouse=True)
def the_default_form_afterwards(engine):
    """the engine is the session's: the tests that run after this file and name no form get the default one, not RESET's"""
    yield
    engine.set_option("s1_skm_deal", 2)


@pytest.mark.parametrize("opts", SETTINGS, ids=ids)
@pytest.mark.parametrize("kind,k,m", LIBRARIES)
@pytest.mark.parametrize("deal", FORMS)
def test_every_form_of_the_dealing(engine, deal, kind, k, m, opts):
    run(engine, fixed_library(kind, seed=k * 13 + m), k, m, dict(opts, s1_skm_deal=deal, s1_skm=2, s1_skm_max_bin=1 << 30))


N_LONG_RUN_READS = 8000


def long_run_reads(k, n=N_LONG_RUN_READS, seed=5):
    """reads of k + 1 + 63 bases, 64 windows each, whose records are long and lie in a few bins.  A read is a tandem repeat of a unit of
    7, 9 or 10 bases: a window holds 10 m-mers (m = k - 8), so every window of the read holds every rotation of the unit and all of them
    share one minimizer — each aligned block of eight windows leaves as ONE record of eight, and all reads of a unit fill one bin whatever
    the number of bins.  Seven reads in ten change to another unit at a random base: the 21 windows across the change have minimizers of
    their own or of either side, which cuts records of 1 to 8 windows at every offset (and makes the keys that occur once, whose marks
    need the window's position).  A wavefront's 64 records then hold well over 256 windows, and their runs cross the chunk boundaries at
    all offsets."""
    rng = np.random.default_rng(seed)
    units = [rng.integers(0, 4, size=p, dtype=np.uint8) for p in (7, 9, 10, 7, 9, 10)]
    assert all(len(set(u.tolist())) > 1 for u in units)
    L = k + 1 + 63

    def repeat_of(u):
        return np.roll(np.tile(u, L // len(u) + 2), int(rng.integers(0, len(u))))[:L]

    reads = []
    for _ in range(n):
        a, b = rng.choice(len(units), size=2, replace=False)
        r = repeat_of(units[a])
        if rng.random() < 0.7:
            cut = int(rng.integers(1, L))
            r = np.concatenate([r[:cut], repeat_of(units[b])[cut:]])
        reads.append(r.astype(np.uint8))
    return reads


LONG_RUN_SETTINGS = [dict(), dict(s1_skm_bin_bits=8), dict(s1_skm_bin_bits=11, s1_skm_tags=1), dict(s1_skm_bin_bits=8, s1_stream_fill=40),
                     dict(s1_skm_bin_bits=8, s1_stream_probes=2)]


@pytest.mark.parametrize("opts", LONG_RUN_SETTINGS, ids=ids)
@pytest.mark.parametrize("k,m", [(21, 2), (22, 1), (19, 2)])
@pytest.mark.parametrize("deal", FORMS)
def test_runs_across_chunk_and_group_boundaries(engine, deal, k, m, opts):
    run(engine, long_run_reads(k), k, m, dict(opts, s1_skm_deal=deal, s1_skm=2, s1_skm_max_bin=1 << 30))


@pytest.mark.parametrize("k", [19, 21, 22])
def test_the_long_run_library_has_wavefronts_of_more_than_256_windows(engine, k):
    """counted from the plan line of the run (records and windows of the job): a wavefront takes 64 consecutive records of one bin, so
    R records in at most 256 bins are at most R / 64 + 256 wavefronts; were none of them beyond 256 windows, the job would hold at
    most 256 (R / 64 + 256) windows"""
    run(engine, long_run_reads(k), k, 2, dict(s1_skm_deal=2, s1_skm_bin_bits=8, s1_skm=2, s1_skm_max_bin=1 << 30))
    plan = engine.last_s1_plan()
    found = re.search(r"2\^8 bins \((\d+) records for (\d+) windows", plan)
    assert found, plan
    records, windows = int(found.group(1)), int(found.group(2))
    print("k = %d: %s" % (k, plan))
    assert windows == N_LONG_RUN_READS * 64, plan
    assert windows > 256 * (records // 64 + 1 + 256), plan
