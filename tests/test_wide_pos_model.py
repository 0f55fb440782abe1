"""CPU: the composition of tests/wide_pos_util.py against the oracle itself.  At T = 2^20 the sparse library B is small enough for the oracle:
what compose_s1 / compose_count make of the compact library C must equal the oracle's answer for B in every field and every bit, and the
spliced packed words and start[] must be those of ob.Package(B) — for every layout tests/test_gpu_skm_past_2_32.py runs at T = 2^32, where
nothing but the GPU can read B."""
import numpy as np
import pytest

import oracle_binding as ob
import wide_pos_util as wp

T20 = 1 << 20


@pytest.fixture(scope="module", params=[(name, kind) for name in wp.LAYOUTS for kind in (("random", "copy") if name == "main" else ("random",))],
                ids=lambda p: "%s-%s" % p)
def pair(request):
    name, kind = request.param
    lay = wp.build(T20, wp.LAYOUTS[name][0], wp.LAYOUTS[name][1], 5, kind)
    return lay, ob.Package(wp.b_reads(lay), reverse=True)


def test_the_spliced_words_are_the_package_of_b(pair):
    lay, pkg = pair
    assert pkg.n_seqs == lay.n_seqs and int(pkg.start()[-1]) == lay.n_bases
    assert np.array_equal(pkg.words(), lay.words)
    start = pkg.start()
    if lay.fixed_len:
        assert np.array_equal(start, np.arange(lay.n_seqs + 1, dtype=np.uint64) * np.uint64(lay.fixed_len))
    else:
        assert np.array_equal(start, lay.start)
    s_at = int(start[lay.c_s + lay.read_shift])
    assert s_at == T20 - lay.off and s_at < T20 <= int(start[lay.c_s + lay.read_shift + 1]) - 1 or lay.off == 0 and s_at == T20
    assert lay.span[0] < T20 < lay.span[1]


@pytest.mark.parametrize("k,m", [(21, 2), (19, 3), (22, 4)])
def test_stage_1_composes(pair, k, m):
    lay, pkg = pair
    want = ob.s1(pkg, k, m, tie_stable=True)
    got = wp.compose_s1(lay, k, m)
    assert got["n_items"] == want["n_items"]
    assert np.array_equal(got["hist"], want["hist"])
    bits = wp.bits_of(want["is_solid"], lay.n_bases)
    assert got["n_solid"] == int(bits.sum()) == wp.popcount(want["is_solid"])
    assert np.array_equal(lay.expected_bits(got["c_bits"], 0, lay.n_bases), bits)
    lo, hi = lay.span
    assert bits[lo:hi].any() and not bits[lo:hi].all()  # (solid and non-solid windows among the reads)


@pytest.mark.parametrize("k,m", [(21, 2), (21, 3), (20, 1)])
def test_count_composes(pair, k, m):
    lay, pkg = pair
    want = ob.count(pkg, k, m)
    got = wp.compose_count(lay, k, m)
    assert got["n_items"] == want["n_items"] and got["wpe"] == want["wpe"]
    assert np.array_equal(got["edges"], want["edges"])
    assert np.array_equal(got["bucket_count"], want["bucket_count"])
    assert np.array_equal(got["hist"], want["hist"])
    for name in ("first_0_out", "last_0_in"):
        assert np.array_equal(wp.expected_per_read(lay, got, name, 0, lay.n_seqs), want[name]), name


def test_stage_2_composes():
    """with 2 (f + f') >= 65536 '$' items in C their runs are at the cap as in B: stage 2 of C is stage 2 of B (T = 2^23: B has room for
    the fillers)"""
    k, m = 21, 2
    lay = wp.build(1 << 23, 150, None, 5, "random", f_post=33000)
    assert 2 * (len(lay.c_reads) - (lay.c_mid[1] - lay.c_mid[0])) >= 65536
    pkg = ob.Package(wp.b_reads(lay), reverse=True)
    assert np.array_equal(pkg.words(), lay.words)
    b1 = ob.s1(pkg, k, m, tie_stable=True)
    got = wp.compose_s1(lay, k, m)
    assert got["n_items"] == b1["n_items"] and np.array_equal(got["hist"], b1["hist"])
    assert np.array_equal(lay.expected_bits(got["c_bits"], 0, lay.n_bases), wp.bits_of(b1["is_solid"], lay.n_bases))
    want, have = ob.s2(pkg, k, m, b1["is_solid"]), ob.s2(lay.c_pkg(), k, m, got["is_solid_c"])
    for name in ("k", "wpt", "ones_in_last"):
        assert have[name] == want[name], name
    for name in ("bytes", "bucket_off", "bucket_items", "bucket_tips", "bucket_large", "w_count"):
        assert np.array_equal(have[name], want[name]), name
