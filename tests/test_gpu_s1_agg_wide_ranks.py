"""GPU: s1_agg_wide on several ranks (comm.hip mhx_dist_read2sdbg) — at k = 23..27 the owner's group-by of the pre-sorted exchange leaves
the compact aggregated items, and stage 2 exchanges those 8-byte items as at k <= 22 instead of per-occurrence ones.  Ranks as threads
on one device behind the in-process transport, as in tests/test_gpu_comm.py; the concatenated streams are the oracle's
(reference src/sorting/read_to_sdbg_s2.cpp:271-440,521-614), also in bucket-range passes."""
import numpy as np
import pytest

import oracle_binding as ob
from megahit_amd import lib
from test_gpu_comm import all_reads, check_sdbg, load_reads, run_ranks, sdbg_of

pytestmark = pytest.mark.gpu

_want = {}


def want_of(world, k, m):
    """the oracle's stage 1 + stage 2 over the ranks' reads together, once per shape"""
    if (world, k, m) not in _want:
        pkg = all_reads(world)
        s1 = ob.s1(pkg, k, m)
        _want[(world, k, m)] = (s1["hist"], ob.s2(pkg, k, m, s1["is_solid"]))
    return _want[(world, k, m)]


@pytest.mark.parametrize("world,k,m,opts", [
    (2, 27, 2, None), (3, 27, 2, None), (2, 23, 3, None), (3, 23, 3, None),
    (3, 27, 2, {"dist_max_items": 40000}),  # bucket-range passes: every pass's items behind those of the passes before it
])
def test_read2sdbg_ranks_with_the_wide_items(world, k, m, opts):
    def body(r, e, cm):
        cm.setup(0, k, m)
        cm.bytes_sent(reset=True)
        cm.read2sdbg(k, m)
        return sdbg_of(e) + (e.fetch(lib.BUF_MUL_HIST, np.int64), e.last_s1_plan(), cm.bytes_sent())

    outs = run_ranks(world, load_reads, body, dict(opts or {}, s1_agg_wide=1))
    hist, want = want_of(world, k, m)
    for o in outs:
        print("plan: %s; %d bytes sent" % (o[5], o[6]))
    assert np.array_equal(sum(o[4] for o in outs), hist)
    check_sdbg(outs, want)
    marker = "[aggregated stage-2 items, %d count bits]" % min(16, 60 - 2 * k)
    for o in outs:
        if "[pre-sorted exchange]" in o[5]:
            assert marker in o[5], o[5]
    assert any(marker in o[5] for o in outs), [o[5] for o in outs]
