"""The banded similarity kernel of the complex bubble remover (include/mhx.h: mhx_unitig_similarity) against a plain Python model
of the reference's GetSimilarity, written from its description: max_indel = int(max(n, m) * (1 - sim)); 0 when |n - m| >
max_indel or max_indel < 1; else the edit distance inside the band of 2 * max_indel + 1 diagonals, with a row-0 of j, a column-0
of i while i <= max_indel, and 0x3f3f3f3f elsewhere; result 1 - d * 1.0 / max(n, m).  Results must be the same doubles, bit for
bit.  The band has 2 * max_indel + 1 cells, always an odd number: the kernel's 64-cell chunks are crossed at max_indel = 31 | 32
(63 | 65 cells) and 63 | 64 (127 | 129 cells), and rows near both ends of the strings have every number of computed cells from
max_indel + 1 up, 64 and 128 among them.  The long cases use a row-vectorised form of the same model, which a CPU test here
holds to the plain one."""
import struct

import numpy as np
import pytest

from megahit_amd import lib

INF = 0x3f3f3f3f


def model(a, b, sim):
    n, m = len(a), len(b)
    d = int(max(n, m) * (1 - sim))
    if abs(n - m) > d or d < 1:
        return 0.0
    prev = [0] * (2 * d + 1)
    for j in range(d + 1):
        prev[j + d] = j
    for i in range(1, n + 1):
        cur = [INF] * (2 * d + 1)
        if i - d <= 0:
            cur[0 - i + d] = i
        for j in range(max(i - d, 1), min(m, i + d) + 1):
            c = j - i + d
            v = min(cur[c], prev[c] + (a[i - 1] != b[j - 1]))
            if j > i - d:
                v = min(v, cur[c - 1] + 1)
            if j < i + d:
                v = min(v, prev[c + 1] + 1)
            cur[c] = v
        prev = cur
    return 1 - prev[m - n + d] * 1.0 / max(n, m)


def model_rows(a, b, sim):
    """the same, one numpy row at a time: the cell to the left is a running minimum of (value - column) + column"""
    n, m = len(a), len(b)
    d = int(max(n, m) * (1 - sim))
    if abs(n - m) > d or d < 1:
        return 0.0
    av, bv = np.frombuffer(a.encode(), np.uint8), np.frombuffer(b.encode(), np.uint8)
    w = 2 * d + 1
    cols = np.arange(w, dtype=np.int64)
    prev = np.where(cols >= d, cols - d, 0)
    for i in range(1, n + 1):
        j = i + cols - d
        inside = (j >= 1) & (j <= m)
        t = np.full(w, INF, dtype=np.int64)
        bj = bv[np.clip(j - 1, 0, max(m - 1, 0))] if m else np.zeros(w, np.uint8)
        diag = prev + (bj != av[i - 1])
        up = np.concatenate([prev[1:] + 1, [INF]])
        t[inside] = np.minimum(np.minimum(t, diag), up)[inside]
        if i <= d:
            t[d - i] = i
        cur = np.full(w, INF, dtype=np.int64)
        lo = d - i if i <= d else 0
        seg = (cols >= lo) & (inside | (cols == lo))
        hi = int(np.nonzero(seg)[0].max()) + 1 if seg.any() else lo
        cur[lo:hi] = np.minimum.accumulate(t[lo:hi] - cols[lo:hi]) + cols[lo:hi]
        prev = cur
    return 1 - int(prev[m - n + d]) * 1.0 / max(n, m)


def rand(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, size=n))


def mutate(s, rng, subs=0, ins=0, dels=0):
    s = list(s)
    for _ in range(subs):
        p = int(rng.integers(0, len(s)))
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
    for _ in range(dels):
        del s[int(rng.integers(0, len(s)))]
    for _ in range(ins):
        s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[int(rng.integers(0, 4))])
    return "".join(s)


def length_for(d, sim):
    """the smallest n with int(n * (1 - sim)) == d"""
    n = 1
    while int(n * (1 - sim)) < d:
        n += 1
    assert int(n * (1 - sim)) == d
    return n


def same_bits(x, y):
    return struct.pack("<d", x) == struct.pack("<d", y)


def test_the_row_model_is_the_plain_model():
    rng = np.random.default_rng(5)
    for _ in range(300):
        sim = float(rng.choice([0.5, 0.8, 0.9, 0.95]))
        n = int(rng.integers(1, 70))
        a = rand(rng, n)
        b = mutate(a, rng, subs=int(rng.integers(0, 4)), ins=int(rng.integers(0, 4)), dels=int(rng.integers(0, min(4, n))))
        if not b:
            b = "A"
        assert same_bits(model(a, b, sim), model_rows(a, b, sim)), (a, b, sim)


def band_cases():
    rng = np.random.default_rng(11)
    out = []
    for d in (31, 32, 63, 64):
        n = length_for(d, 0.95)
        a = rand(rng, n)
        out.append(("d%d-edits" % d, a, mutate(a, rng, subs=5, ins=3, dels=3), 0.95))
        out.append(("d%d-many-edits" % d, a, mutate(a, rng, subs=n // 10, ins=d // 2, dels=d // 2), 0.95))
        out.append(("d%d-shorter-by-d" % d, a, mutate(a, rng, dels=d), 0.95))         # n - m = max_indel
        out.append(("d%d-shorter-by-d+1" % d, a, mutate(a, rng, dels=d + 1), 0.95))   # one past: 0
        out.append(("d%d-longer-by-d" % d, mutate(a, rng, dels=d), a, 0.95))          # n - m = -max_indel
        out.append(("d%d-longer-by-d+1" % d, mutate(a, rng, dels=d + 1), a, 0.95))
        out.append(("d%d-prefix" % d, a, a[:n - d], 0.95))                            # all the indels at the end
        out.append(("d%d-suffix" % d, a, a[d:], 0.95))                                # ... at the start
    return out


def small_cases():
    rng = np.random.default_rng(12)
    out = []
    for n in (1, 2, 3):
        for m in (1, 2, 3):
            for sim in (0.1, 0.34, 0.5, 0.67):
                a, b = rand(rng, n), rand(rng, m)
                out.append(("n%d-m%d-s%s" % (n, m, sim), a, b, sim))
                out.append(("n%d-m%d-s%s-A" % (n, m, sim), "A" * n, "A" * m, sim))
    a = rand(rng, 19)
    out.append(("max_indel-0", a, a, 0.95))                       # int(19 * 0.05) = 0: 0 even for equal strings
    a = rand(rng, 20)
    out.append(("max_indel-1-equal", a, a, 0.95))
    out.append(("max_indel-1-snp", a, mutate(a, rng, subs=1), 0.95))
    out.append(("max_indel-1-first-deleted", a, a[1:], 0.95))
    out.append(("max_indel-1-last-deleted", a, a[:-1], 0.95))
    out.append(("max_indel-1-first-inserted", a, "T" + a, 0.95))   # max(n, m) = 21: still 1
    out.append(("max_indel-1-two-shorter", a, a[2:], 0.95))        # |n - m| > max_indel
    a = rand(rng, 400)
    out.append(("identical", a, a, 0.95))
    out.append(("all-mismatch", "A" * 400, "C" * 400, 0.95))
    out.append(("all-mismatch-shifted", "AC" * 200, "CA" * 200, 0.95))
    out.append(("first-deleted", a, a[1:], 0.95))
    out.append(("last-deleted", a, a[:-1], 0.95))
    out.append(("first-inserted", "G" + a, a, 0.95))
    out.append(("last-inserted", a + "G", a, 0.95))
    out.append(("reverse-complement", a, a[::-1].translate(str.maketrans("ACGT", "TGCA")), 0.95))  # the strands a pair may be on
    return out


CASES = band_cases() + small_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_similarity_is_the_models_double(engine, case):
    _, a, b, sim = case
    want = model(a, b, sim)
    got = engine.unitig_similarity(a, b, sim)
    assert same_bits(got, want), (got, want, len(a), len(b), int(max(len(a), len(b)) * (1 - sim)))


def test_the_cases_cover_what_they_are_for():
    """non-vacuity of the list above (no device work)"""
    def d_of(c):
        return int(max(len(c[1]), len(c[2])) * (1 - c[3]))

    assert {d_of(c) for c in CASES if c[0].endswith("-edits")} == {31, 32, 63, 64}
    assert all(model(c[1], c[2], c[3]) == 0.0 for c in CASES if c[0].endswith("by-d+1"))
    assert all(0 < model(c[1], c[2], c[3]) < 1 for c in CASES if c[0].endswith("by-d") or c[0].endswith("fix"))
    assert any(0 < model(c[1], c[2], c[3]) < 1 for c in CASES if c[0].startswith("n"))
    by = {c[0]: c for c in CASES}
    assert model(*by["identical"][1:]) == 1.0 and model(*by["max_indel-0"][1:]) == 0.0 and model(*by["all-mismatch"][1:]) == 0.0
    assert model(*by["max_indel-1-two-shorter"][1:]) == 0.0 and model(*by["max_indel-1-first-inserted"][1:]) > 0.9


@pytest.mark.gpu
def test_the_cap_and_one_past_it(engine):
    """strings of MHX_SIM_MAX_LEN characters and a band of MHX_SIM_MAX_INDEL run; one more of either is an error"""
    rng = np.random.default_rng(13)
    a = rand(rng, lib.SIM_MAX_LEN)
    b = mutate(a, rng, subs=40, ins=15, dels=25)
    assert len(b) <= lib.SIM_MAX_LEN
    assert same_bits(engine.unitig_similarity(a, b, 0.98), model_rows(a, b, 0.98))
    with pytest.raises(lib.MhxError, match="MHX_SIM_MAX_LEN"):
        engine.unitig_similarity(a + "A", b, 0.98)
    with pytest.raises(lib.MhxError, match="MHX_SIM_MAX_LEN"):
        engine.unitig_similarity(b, a + "A", 0.98)
    n = 2 * lib.SIM_MAX_INDEL  # int(n * 0.5) = MHX_SIM_MAX_INDEL: 4095 cells, 64 chunks
    a = rand(rng, n)
    b = mutate(a, rng, subs=300, ins=200, dels=260)
    assert int(max(len(a), len(b)) * 0.5) == lib.SIM_MAX_INDEL
    assert same_bits(engine.unitig_similarity(a, b, 0.5), model_rows(a, b, 0.5))
    with pytest.raises(lib.MhxError, match="MHX_SIM_MAX_INDEL"):
        engine.unitig_similarity(a + "AC", b, 0.5)
    for bad in (0.0, -1.0, 1.5):
        with pytest.raises(lib.MhxError, match="similarity"):
            engine.unitig_similarity("ACGT", "ACGT", bad)
