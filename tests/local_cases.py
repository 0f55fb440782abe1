"""The inputs of the `local` mapping tests, made from seeds: contigs cut from a random genome and read libraries over it.

build(case) -> (contigs as the FASTA file holds them: [(bases uint8, flag)], libraries: [(reads: list of uint8 arrays, paired)]).
A case is a dict(name, seed, seed_kmer, sparsity, min_mapping_len, similarity); tests/golden/local_map.json holds the cases with
the numbers the reference logged for them (tools/make_local_golden.py).  Contig flags: 1 standalone, 2 loop.
"""
import os

import numpy as np

from megahit_amd import synth

MIN_CONTIG_LEN = 200


def rc(x):
    return (3 - np.asarray(x, dtype=np.uint8))[::-1].copy()


def _errors(rng, read, err):
    read = np.array(read, dtype=np.uint8)
    if err > 0:
        mask = rng.random(read.size) < err
        read[mask] = (read[mask] + rng.integers(1, 4, size=int(mask.sum()), dtype=np.uint8)) & 3
    return read


def _pairs(rng, genome, n_pairs, len1, len2, frag, err):
    out = []
    for s in rng.integers(0, genome.size - frag, size=n_pairs):
        out.append(_errors(rng, genome[s:s + len1], err))
        out.append(_errors(rng, rc(genome[s + frag - len2:s + frag]), err))
    return out


def _singles(rng, genome, n, length, err):
    out = []
    for s in rng.integers(0, genome.size - length, size=n):
        r = genome[s:s + length]
        out.append(_errors(rng, rc(r) if rng.random() < 0.5 else r, err))
    return out


def _cut(genome, bounds, flags=None):
    return [(genome[a:b].copy(), (flags or {}).get(i, 0)) for i, (a, b) in enumerate(bounds)]


def _pe150(rng):
    """paired reads of 150 bases with 3 % errors over contigs with gaps between them: mates on the same contig, on different contigs and
    unmapped; a contig of exactly 200 bases (shorter than the local range), one of 199 (dropped) and a loop contig (dropped: ids shift)"""
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)
    contigs = _cut(g, [(0, 900), (1000, 1200), (1250, 1449), (1500, 2600), (2650, 2950), (3000, 4000)], {4: 2, 0: 1})
    reads = [r for r in synth.gen_pe_reads(300, g.size, read_len=150, frag=320, err=0.03, seed=int(rng.integers(1 << 30)), genome=g)]
    return contigs, [(reads, True)]


def _lengths(rng):
    """error-free pairs of every length at a word edge of the match count or a chunk edge of the positions, and reads shorter than the seed"""
    g = rng.integers(0, 4, size=3000, dtype=np.uint8)
    contigs = _cut(g, [(0, 1400), (1450, 3000)])
    reads = []
    for n in (20, 30, 49, 50, 63, 64, 65, 95, 150, 151):
        reads += _pairs(rng, g, 12, n, n, 330, 0.0)
    reads += _pairs(rng, g, 20, 151, 64, 300, 0.03)
    return contigs, [(reads, True)]


def _noisy_single(rng):
    """a single-end library with 0 %, 3 % and 25 % errors: the similarity threshold is crossed both ways, 15 and more mismatches"""
    g = rng.integers(0, 4, size=2500, dtype=np.uint8)
    contigs = _cut(g, [(0, 1200), (1300, 2500)])
    reads = _singles(rng, g, 80, 100, 0.0) + _singles(rng, g, 120, 100, 0.03) + _singles(rng, g, 250, 100, 0.25) + _singles(rng, g, 150, 100, 0.18)
    # 150 bases with 45 clean ones in a row (room for a sampled seed) and 15 / 22 / 30 % errors in the rest: 15 and more mismatches that
    # pass, and counts either side of lround(0.8 * 150) = 120
    for err in (0.15, 0.22, 0.30):
        for r in _singles(rng, g, 60, 150, 0.0):
            at = int(rng.integers(0, 105))
            noisy = _errors(rng, r, err)
            noisy[at:at + 45] = r[at:at + 45]
            reads.append(noisy)
    order = rng.permutation(len(reads))
    return contigs, [([reads[i] for i in order], False)]


def _overhang(rng):
    """reads of 150 bases that hang over either end of a contig with 1, 74, 75, 76 and 120 bases on it, both strands"""
    g = rng.integers(0, 4, size=3000, dtype=np.uint8)
    bounds = [(200, 1100), (1400, 2800)]
    contigs = _cut(g, bounds)
    reads = []
    for a, b in bounds:
        for on in (1, 74, 75, 76, 120):
            for rep in range(3):
                left = g[a + on - 150:a + on]  # `on` bases on the contig's start
                right = g[b - on:b - on + 150]
                for r in (left, right):
                    r = _errors(rng, r, 0.01 * rep)
                    reads.append(r)
                    reads.append(rc(r))
    return contigs, [(reads, False)]


def _repeat(rng):
    """an exact repeat of 300 bases shared by two contigs: its seeds are flagged; reads inside it find nothing, reads across its edge
    map through the seeds beside it"""
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)
    g[2500:2800] = g[600:900]
    contigs = _cut(g, [(0, 1800), (1900, 4000)])
    reads = _pairs(rng, g, 250, 100, 100, 280, 0.01)
    return contigs, [(reads, True)]


def _rc_ends(rng):
    """the last 260 bases of contig 1 are the reverse complement of the last 260 of contig 0, placed so that the sampled seeds of the
    two do not coincide at sparsity 8 (nothing flagged: reads inside map to both with equal counts -> invalid)"""
    g = rng.integers(0, 4, size=1400, dtype=np.uint8)
    c0 = g[:700].copy()
    c1 = np.concatenate([g[800:1244], rc(c0[440:700])])  # 704 bases: a window at j >= 444 is c0's at 1113 - j, never both multiples of 8
    reads = []
    for s in rng.integers(380, 560, size=120):
        r = _errors(rng, c0[s:s + 120], 0.0 if s % 2 else 0.02)
        reads.append(rc(r) if s % 3 == 0 else r)
    for s in rng.integers(0, 450, size=60):
        reads.append(_errors(rng, c1[s:s + 120], 0.01))
    return [(c0, 0), (c1, 0)], [(reads, False)]


def _two_libs(rng):
    """a paired and a single-end library in one collection: different local ranges"""
    g = rng.integers(0, 4, size=3500, dtype=np.uint8)
    contigs = _cut(g, [(0, 1000), (1100, 1400), (1500, 3500)])
    return contigs, [(_pairs(rng, g, 150, 100, 100, 260, 0.02), True), (_singles(rng, g, 200, 120, 0.02), False)]


def _no_contig(rng):
    """no contig is kept: an empty index, nothing maps"""
    g = rng.integers(0, 4, size=2000, dtype=np.uint8)
    contigs = _cut(g, [(0, 150), (200, 399), (500, 1500)], {2: 2})
    return contigs, [(_pairs(rng, g, 100, 100, 100, 250, 0.01), True)]


def _two_batches(rng):
    """2^19 + 2^18 + 1000 reads of 60 bases, error-free over one contig, so that every pair counts: the histogram is full after exactly two
    batches of 2^18 reads.  From read 2^19 on the fragments are 100 bases longer: an estimate that reads on gives another mean"""
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)
    seeds = rng.integers(1 << 30, size=2)
    a = synth.gen_pe_reads(1 << 18, g.size, read_len=60, frag=200, err=0.0, seed=int(seeds[0]), genome=g)
    b = synth.gen_pe_reads((1 << 17) + 500, g.size, read_len=60, frag=300, err=0.01, seed=int(seeds[1]), genome=g)
    return [(g.copy(), 0)], [(np.concatenate([a, b]), True)]


def _seed32(rng, dup):
    """for seeds of 32 bases, whose keys use all 64 bits: a run of exactly 32 T in contig 0 at a sampled offset (its canonical key is 0, the
    reverse complement 32 A), a 32-base window equal to its own reverse complement, and the keys with bit 63 set that random sequence
    gives (a quarter of them).  dup: a run of exactly 32 A in contig 1 as well, so that key 0 is flagged and never used"""
    g = rng.integers(0, 4, size=3000, dtype=np.uint8)
    g[399], g[400:432], g[432] = 1, 3, 2
    half = g[800:816].copy()
    g[816:832] = rc(half)
    if dup:
        g[1999], g[2000:2032], g[2032] = 1, 0, 2  # offset 496 of contig 1
    contigs = _cut(g, [(0, 1400), (1504, 3000)])
    reads = _pairs(rng, g, 150, 100, 100, 280, 0.01)
    for s in rng.integers(250, 420, size=40):  # pairs whose first mate covers the run of T (and, every other one, starts inside it)
        reads.append(_errors(rng, g[s:s + 100], 0.0))
        reads.append(_errors(rng, rc(g[s + 180:s + 280]), 0.01))
    for s in rng.integers(740, 800, size=20):  # ... the self-complementary window
        reads.append(_errors(rng, g[s:s + 100], 0.0))
        reads.append(_errors(rng, rc(g[s + 180:s + 280]), 0.0))
    for s in (400, 401, 1904 + 96):  # reads that begin with the run itself
        reads.append(g[s:s + 100].copy())
        reads.append(rc(g[s + 150:s + 250]))
    return contigs, [(reads, True)]


BUILDERS = {"seed32": lambda rng: _seed32(rng, False), "seed32_dup": lambda rng: _seed32(rng, True),
            "pe150": _pe150, "lengths": _lengths, "noisy_single": _noisy_single, "overhang": _overhang, "repeat": _repeat, "rc_ends": _rc_ends,
            "two_libs": _two_libs, "no_contig": _no_contig, "two_batches": _two_batches}
LARGE = ("two_batches",)  # compared with the golden numbers only: too many reads for the model


def build(case):
    return BUILDERS[case["name"]](np.random.default_rng(case["seed"]))


def read_lengths(libs):
    """-> uint32 [n_reads]"""
    out = [np.full(r.shape[0], r.shape[1], dtype=np.uint32) if isinstance(r, np.ndarray) else np.array([len(x) for x in r], dtype=np.uint32)
           for r, _ in libs]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


def lib_table(libs):
    """-> [(begin, end, max length, paired)] as the lines of .lib_info"""
    out, at = [], 0
    for reads, paired in libs:
        lens = read_lengths([(reads, paired)])
        out.append((at, at + lens.size, int(lens.max()) if lens.size else 0, bool(paired)))
        at += lens.size
    return out


def all_reads(libs):
    return [r for reads, _ in libs for r in reads]


def bin_records(libs):
    """the `.bin` record stream of the libraries (uint32: per read its length + packed words)"""
    out = []
    for reads, _ in libs:
        if isinstance(reads, np.ndarray):
            n, L = reads.shape
            rec = np.empty((n, 1 + (L + 15) // 16), dtype=np.uint32)
            rec[:, 0] = L
            rec[:, 1:] = synth.pack_reads(reads)
            out.append(rec.reshape(-1))
        else:
            for r in reads:
                out.append(np.array([len(r)], dtype=np.uint32))
                out.append(synth.pack_reads(np.asarray(r, dtype=np.uint8)[None, :])[0])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


def pack_contigs(kept):
    """-> (packed words, start offsets) of the kept contigs, as mhx_local_index takes them"""
    start = np.zeros(len(kept) + 1, dtype=np.uint64)
    for i, c in enumerate(kept):
        start[i + 1] = start[i] + len(c)
    flat = np.concatenate(kept) if kept else np.zeros(0, dtype=np.uint8)
    return (synth.pack_reads_concat(flat[None, :]) if flat.size else np.zeros(0, dtype=np.uint32)), start


def write_files(case, directory):
    """contigs FASTA (+ .info) and the read library (.bin + .lib_info) of a case -> (fasta path, library prefix)"""
    contigs, libs = build(case)
    fa = os.path.join(directory, case["name"] + ".contigs.fa")
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(fa, "w") as f:
        for i, (c, flag) in enumerate(contigs):
            f.write(">k21_%d flag=%d multi=10.0000 len=%d\n%s\n" % (i, flag, len(c), lut[c].tobytes().decode()))
    with open(fa + ".info", "w") as f:
        f.write("%d %d\n" % (len(contigs), sum(len(c) for c, _ in contigs)))
    prefix = os.path.join(directory, case["name"] + ".lib")
    bin_records(libs).tofile(prefix + ".bin")
    table = lib_table(libs)
    with open(prefix + ".lib_info", "w") as f:
        f.write("%d %d\n" % (int(read_lengths(libs).sum(dtype=np.int64)), table[-1][1]))
        for b, e, m, p in table:
            f.write("synthetic\n%d %d %d %d\n" % (b, e, m, int(p)))
    return fa, prefix
