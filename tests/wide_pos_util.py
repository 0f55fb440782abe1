"""A sparse library with a read across base position T (2^32 in tests/test_gpu_skm_past_2_32.py, 2^20 in tests/test_wide_pos_model.py) and the
oracle's answer for it, composed from the oracle's answer for a compact library.  No GPU in here.

    B = [D filler units] + C            C = [f poly-A reads] + X + [S] + X' + [f' poly-A reads]

X and X' are a few thousand synthetic reads, S is the one read that starts at T - off.  A filler unit is one poly-A read of L bases (fixed
length) or two of `hi` and `hi - 1` bases (several lengths; six more poly-A reads in front of X take what is left to T - off).  D is a multiple
of 16, so the packed words of B are zeros with the words of C's tail spliced in at a word boundary: B at T = 2^32 costs a lazily zero
np.zeros of 1.07 GB and no oracle run.  Poly-A windows are one key; where its count is at the cap of 65535 in C already, the histogram, the
edges and the bucket counts of B are those of C, the marks of X, S, X' are C's moved by D units, every filler read looks like C's, and the
item count grows by a fixed amount per unit (the oracle's own: C minus C without its first unit).
"""
import numpy as np

import oracle_binding as ob
from megahit_amd import synth
from test_gpu_skm_rep import stretch_read

K0 = 21  # the k the lone windows are cut for
CAP = 65535
A, C, G, T = 0, 1, 2, 3
# layout -> (lengths, off); off None: T mod L, the only value a library of one length can have
LAYOUTS = {"main": (150, None), "early": (151, None), "block edge": (120, None), "aligned": (128, None), "var last": ((60, 150), "last"),
           "var first": ((60, 150), "first")}


def _pe(rng, n_pairs, genome, length):
    return [r for r in synth.gen_pe_reads(n_pairs, genome.size, read_len=length, frag=min(300, 2 * length), err=0.01, seed=int(rng.integers(1 << 30)), genome=genome)]


def _content(rng, genome, length, special, n_pe=600, n_embedded=300):
    """reads of `length` bases: PE reads with errors over a small genome (solid and non-solid windows alternate inside a read), random reads
    seen once, twice and three times (keys of count exactly 1, 2, 3), reads with an embedded (AC)x20 stretch; special: 1500 of those, one
    read with the only window of K0 + 1 C's and one with the only (ACG)n window of K0 + 1 bases"""
    out = _pe(rng, n_pe, genome, length)
    out += [rng.integers(0, 4, size=length, dtype=np.uint8) for _ in range(150)]
    for copies in (2, 3):
        for _ in range(60):
            r = rng.integers(0, 4, size=length, dtype=np.uint8)
            out += [r.copy() for _ in range(copies)]
    out += [out[int(i)].copy() for i in rng.integers(0, 2 * n_pe, size=100)]  # exact duplicates of reads with errors
    for _ in range(1500 if special else n_embedded):
        out.append(stretch_read(rng, [A, C], 40, int(rng.integers(2, length - 42)), length=length))
    if special:
        r = rng.integers(0, 4, size=length, dtype=np.uint8)
        r[20:20 + K0 + 1] = C
        r[19], r[20 + K0 + 1] = A, T
        out.append(r)
        out.append(stretch_read(rng, [A, C, G], K0 + 1, 25, length=length))
    order = rng.permutation(len(out))
    return [out[int(i)] for i in order]


def _mix(c):
    h = (c * 0x9E3779B1) & 0xFFFFFFFF
    return h ^ (h >> 15)


def same_minimizer(stored, k, w0, w1):
    """windows w0 and w1 of a read as the store holds it (ob.Package(reverse=True): the read reversed) share their minimizer, as k_skm_make
    (megahit_amd/csrc/s1_skm.hip) finds it: the smallest _mix(canonical code) among the ten (k - 8)-mers of a window"""
    M = k - 8

    def code(b):
        c = 0
        for v in b:
            c = c * 4 + int(v)
        return c

    def hashes(w):
        return [_mix(min(code(stored[i:i + M]), code(3 - stored[i:i + M][::-1]))) for i in range(w, w + 10)]

    return min(hashes(w0)) == min(hashes(w1))


class Layout:
    """what build() returns: B's packed words (`words`), `fixed_len` or `start`, the compact library (`c_reads`, `c_pkg()`), and the mapping"""

    def expected_bits(self, c_bits, lo, hi):
        """is_solid of B over base positions [lo, hi) as a bool array, from the bool array of C's bits"""
        shift = self.D * self.unit_bases
        out = np.empty(hi - lo, dtype=bool)
        n_fill = max(0, min(hi, shift) - lo)
        if n_fill:
            unit = c_bits[: self.unit_bases]
            out[:n_fill] = unit[(lo + np.arange(n_fill, dtype=np.int64)) % self.unit_bases]
        if hi > shift:
            out[n_fill:] = c_bits[max(lo, shift) - shift: hi - shift]
        return out

    def c_pkg(self):
        if self._pkg is None:
            self._pkg = ob.Package(self.c_reads, reverse=True)
        return self._pkg

    def load(self, engine):
        if self.fixed_len:
            engine.load_sequences(self.words, self.n_seqs, self.fixed_len, None)
        else:
            engine.load_sequences(self.words, self.n_seqs, 0, self.start)


def build(T_at, lengths, off, seed, s_kind, f_pre=640, f_post=64):
    """lengths: L (one length; off must be T_at mod L) or (lo, hi) (X, S, X' of lo..hi bases, fillers of hi and hi - 1); off: the bases of S
    below T_at — or "last" / "first": only S's last window at T_at / only its first below; s_kind: "random" (S is seen nowhere else) or
    "copy" (S is a read of X that is seen nowhere else).  f_pre: the fillers C has in front at least, f_post: those behind"""
    rng = np.random.default_rng([seed, 20])
    var = not isinstance(lengths, int)
    hi = lengths[1] if var else lengths
    genome = rng.integers(0, 4, size=5000, dtype=np.uint8)
    x = _content(rng, genome, hi, special=False)
    xp = _content(rng, genome, hi, special=True)
    if var:  # every read cut to a length of its own (the lone windows lie in the first lo bases; an (AC) stretch may be cut short)
        x = [r[: int(rng.integers(lengths[0], hi + 1))] for r in x]
        xp = [r[: int(rng.integers(lengths[0], hi + 1))] for r in xp]
    s_len = hi
    if var:
        s_len = int(rng.integers(lengths[0] + 40, hi - 8))
        while (s_len - K0 - 1) % 8 == 0:  # ("last": the last window is not alone in its block)
            s_len += 1
    if off is None:
        off = T_at % hi
    elif off == "last":
        off = s_len - K0 - 1
    elif off == "first":
        off = 1
    # S: random bases — taken until the window at T and the one below it share a minimizer at every k (where they lie in one block of eight):
    # a record then runs across T, and the windows past T get their place from the carry into the tag
    for _ in range(1000):
        s = rng.integers(0, 4, size=s_len, dtype=np.uint8)
        if off % 8 == 0 or all(off >= s_len - k or same_minimizer(s[::-1], k, off - 1, off) for k in (19, 20, 21, 22)):
            break
    else:
        raise AssertionError("no S with a record across T")
    if s_kind == "copy":
        x.insert(int(rng.integers(0, len(x))), s.copy())
    x_bases = sum(len(r) for r in x)
    unit = [hi, hi - 1] if var else [hi]
    U = sum(unit)
    R = T_at - off - x_bases  # the bases of all fillers in front of X
    if var:
        n_units = R // U - 2
        rest = R - n_units * U
        adj = [rest // 6 + (1 if i < rest % 6 else 0) for i in range(6)]
        assert all(K0 + 1 <= a <= hi for a in adj), adj
    else:
        assert R % U == 0, "off must be T mod L"
        n_units, adj = R // U, []
    f_units = -(-f_pre // len(unit))
    D = (n_units - f_units) // 16 * 16
    assert D > 0, "T too small for X and the fillers"
    c_units = n_units - D
    fill = lambda lens: [np.zeros(n, dtype=np.uint8) for n in lens]
    mid = x + [s] + xp
    lay = Layout()
    lay._pkg = None
    lay.T, lay.off, lay.var, lay.D, lay.unit, lay.unit_bases = T_at, off, var, D, unit, U
    lay.c_reads = fill(unit * c_units + adj) + mid + fill(unit * (-(-f_post // len(unit))))
    lay.c_lens = np.array([len(r) for r in lay.c_reads], dtype=np.uint64)
    lay.c_start = np.concatenate([[0], np.cumsum(lay.c_lens)]).astype(np.uint64)
    lay.n_adj = len(adj)
    lay.c_fill_pre = c_units * len(unit) + len(adj)  # reads
    lay.c_mid = (lay.c_fill_pre, lay.c_fill_pre + len(mid))  # reads of X, S, X' in C
    lay.c_s = lay.c_fill_pre + len(x)
    lay.read_shift, lay.base_shift = D * len(unit), D * U
    lay.n_seqs = len(lay.c_reads) + lay.read_shift
    lay.n_bases = int(lay.c_start[-1]) + lay.base_shift
    lay.span = (int(lay.c_start[lay.c_mid[0]]) + lay.base_shift, int(lay.c_start[lay.c_mid[1]]) + lay.base_shift)  # base positions of X, S, X' in B
    assert int(lay.c_start[lay.c_s]) + lay.base_shift == T_at - off
    assert lay.base_shift % 16 == 0
    # the packed words: zeros, C's words from its first non-filler word on spliced in
    cw = lay.c_pkg().words()
    assert np.array_equal(lay.c_pkg().start(), lay.c_start)
    w0 = int(lay.c_start[lay.c_mid[0]]) // 16
    assert not cw[:w0].any()
    lay.words = np.zeros((lay.n_bases + 15) // 16 + 1, dtype=np.uint32)
    lay.words[lay.base_shift // 16 + w0: lay.base_shift // 16 + cw.size] = cw[w0:]
    if var:
        lay.fixed_len = 0
        lay.start = np.empty(lay.n_seqs + 1, dtype=np.uint64)
        pre = np.arange(D, dtype=np.uint64) * np.uint64(U)
        lay.start[0: lay.read_shift: 2] = pre
        lay.start[1: lay.read_shift: 2] = pre + np.uint64(hi)
        lay.start[lay.read_shift:] = lay.c_start + np.uint64(lay.base_shift)
    else:
        lay.fixed_len, lay.start = hi, None
    return lay


def b_reads(lay):
    """B read by read (for the oracle at a small T)"""
    return [np.zeros(n, dtype=np.uint8) for n in lay.unit * lay.D] + lay.c_reads


def bits_of(words, n_bits=None):
    """uint64 bitmap words -> bool array, bit p = (words[p >> 6] >> (p & 63)) & 1"""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little").view(bool)
    return b if n_bits is None else b[:n_bits]


def popcount(words):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return int(np.bitwise_count(w).sum(dtype=np.int64))
    table = np.array([bin(i).count("1") for i in range(65536)], dtype=np.uint8)
    return sum(int(table[w[lo: lo + (1 << 23)].view(np.uint16)].sum(dtype=np.int64)) for lo in range(0, w.size, 1 << 23))


def _without_first_unit(lay):
    return ob.Package(lay.c_reads[len(lay.unit):], reverse=True)


def compose_s1(lay, k, m):
    """the oracle's stage 1 of C -> what B must give: n_items, n_solid, hist, `c_bits` (C's is_solid as bools; Layout.expected_bits maps
    a range of B onto it and onto the filler unit's pattern)"""
    c = ob.s1(lay.c_pkg(), k, m, tie_stable=True)
    n_c = int(lay.c_start[-1])
    bits = bits_of(c["is_solid"], n_c)
    U = lay.unit_bases
    n_units_c = (lay.c_fill_pre - lay.n_adj) // len(lay.unit)
    units = bits[: n_units_c * U].reshape(n_units_c, U)
    assert (units == units[0]).all(), "C's filler reads do not all look alike"
    # the cap: the poly-A key's count is 65535 in C as it is in B — the windows of C's fillers alone reach it, and the oracle's histogram has it there
    n_poly = sum(int(n) - k for i, n in enumerate(lay.c_lens) if (i < lay.c_mid[0] or i >= lay.c_mid[1]) and n > k)
    assert n_poly >= CAP and c["hist"][CAP] >= 1, (n_poly, c["hist"][CAP])
    per_unit = c["n_items"] - ob.s1(_without_first_unit(lay), k, m, tie_stable=True)["n_items"]
    return dict(n_items=c["n_items"] + lay.D * per_unit, n_solid=int(bits.sum()) + lay.D * int(units[0].sum()), hist=c["hist"], c_bits=bits,
                is_solid_c=c["is_solid"])


def compose_count(lay, k, m):
    """the oracle's count of C -> what B must give: n_items, wpe, edges, bucket_count, hist, and first_0_out / last_0_in as (the one value of
    a filler read of each place in the unit, the values of C's reads from the first of X on ... to the end)"""
    c = ob.count(lay.c_pkg(), k, m)
    n_poly = sum(int(n) - k for i, n in enumerate(lay.c_lens) if (i < lay.c_mid[0] or i >= lay.c_mid[1]) and n > k)
    assert n_poly >= CAP and c["hist"][CAP] >= 1, (n_poly, c["hist"][CAP])
    nu = len(lay.unit)
    n_units_c = (lay.c_fill_pre - lay.n_adj) // nu
    out = dict(n_items=c["n_items"] + lay.D * (c["n_items"] - ob.count(_without_first_unit(lay), k, m)["n_items"]), wpe=c["wpe"], edges=c["edges"],
               bucket_count=c["bucket_count"], hist=c["hist"])
    for name in ("first_0_out", "last_0_in"):
        v = c[name]
        fill = v[: n_units_c * nu].reshape(n_units_c, nu)
        assert (fill == fill[0]).all(), "C's filler reads do not all have one %s" % name
        out[name + "_unit"] = fill[0].copy()
        out[name + "_c"] = v
    return out


def expected_per_read(lay, comp, name, lo, hi):
    """first_0_out / last_0_in of B's reads [lo, hi)"""
    out = np.empty(hi - lo, dtype=np.uint32)
    n_fill = max(0, min(hi, lay.read_shift) - lo)
    if n_fill:
        out[:n_fill] = comp[name + "_unit"][(lo + np.arange(n_fill)) % len(lay.unit)]
    if hi > lay.read_shift:
        out[n_fill:] = comp[name + "_c"][max(lo, lay.read_shift) - lay.read_shift: hi - lay.read_shift]
    return out
