"""BGZF fixtures for the GPU inflate (megahit_amd/csrc/inflate.hip, inflate_core.h, bgzf_scan.h): a BGZF block / file writer over
zlib's raw deflate, a small DEFLATE bit writer for streams zlib's compressor never emits, the well-formed fixtures with their texts and
the malformed ones with the reason the scan or the decoder must give.  tests/test_bgzf_fixtures.py holds the fixtures to zlib itself."""
import gzip
import struct
import zlib
from collections import namedtuple

import numpy as np

# enum mhx_bgzf_reason (include/mhx.h; test_bgzf_fixtures.py compares)
REASONS = dict(OK=0, NOT_GZIP=1, FLG=2, NO_BC=3, SHORT_BLOCK=4, PAST_EOF=5, TRAILING=6, ISIZE=7, PAYLOAD_END=8, BTYPE=9, STORED_LEN=10,
               CODE_OVER=11, CODE_INCOMPLETE=12, BAD_SYMBOL=13, DIST_FAR=14, OUT_OVER=15, OUT_SHORT=16, CRC=17)

Good = namedtuple("Good", "name data text n_blocks")
Bad = namedtuple("Bad", "name data reason block zlib_raises")


# ---- BGZF ----------------------------------------------------------------------------------------------------------------------------

def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(text) + co.flush()


def block(text, payload=None, crc=None, isize=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """one BGZF member; payload / crc / isize override what `text` gives"""
    if payload is None:
        payload = deflate(text, level, strategy)
    total = 18 + len(payload) + 8
    assert total <= 65536, total
    head = b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + payload + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


EOF_BLOCK = block(b"")


def bgzf(text, block_size=65280, level=6, eof=True):
    out = [block(text[i:i + block_size], level=level) for i in range(0, len(text), block_size)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


# ---- DEFLATE by hand -----------------------------------------------------------------------------------------------------------------

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code over all 19 code-length symbols: 13 of four bits, 6 of five
CL_LENS = [4] * 13 + [5] * 6


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, k):
        """k bits of v, least significant first (extra bits, header fields)"""
        assert 0 <= v < (1 << k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, length):
        """a Huffman code, most significant bit first"""
        for i in range(length - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2); makes no judgement on the set"""
    codes, code = {}, 0
    for length in range(1, 16):
        for s, l in enumerate(lens):
            if l == length:
                codes[s] = (code, length)
                code += 1
        code <<= 1
    return codes


def len_code(length):
    c = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
    return c, length - LEN_BASE[c]


def dist_code(dist):
    c = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return c, dist - DIST_BASE[c]


def put_tokens(w, tokens, lit_lens, dist_lens, eob=True):
    """tokens: a literal byte (int) or (length, distance); then the end-of-block code"""
    lit, dst = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            c, x = len_code(t[0])
            w.code(*lit[257 + c])
            w.bits(x, LEN_EXTRA[c])
            c, x = dist_code(t[1])
            w.code(*dst[c])
            w.bits(x, DIST_EXTRA[c])
    if eob:
        w.code(*lit[256])


def fixed_block(w, tokens, final=True, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST, eob)


def plain_cl_seq(lens):
    """one code-length symbol per length: no repeat codes"""
    return [(l, 0) for l in lens]


def dynamic_block(w, lit_lens, dist_lens, tokens, cl_seq=None, final=True):
    """lit_lens: 257 .. 286 lengths, dist_lens: 1 .. 30; cl_seq: [(code-length symbol, extra value)] spelling lit_lens + dist_lens"""
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    if cl_seq is None:
        cl_seq = plain_cl_seq(list(lit_lens) + list(dist_lens))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for s, x in cl_seq:
        w.code(*cl[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, lit_lens, dist_lens)


def expand(tokens):
    """the text a token list spells"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def lens_of(pairs, n):
    lens = [0] * n
    for s, l in pairs:
        lens[s] = l
    return lens


# ---- texts ---------------------------------------------------------------------------------------------------------------------------

def fastq_text(n_rec, read_len, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_rec):
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=read_len, p=[0.245, 0.245, 0.245, 0.245, 0.02]))
        # quality lines as sequencers write them: long runs of one value
        q = bytearray()
        while len(q) < read_len:
            q += bytes([int(rng.choice([70, 70, 70, 58, 44, 35]))]) * int(rng.integers(1, 40))
        out.append(b"@r%d\n%s\n+\n%s\n" % (i, seq, bytes(q[:read_len])))
    return b"".join(out)


_cache = {}


def records_1000():
    if "r1000" not in _cache:
        _cache["r1000"] = fastq_text(1000, 20, 11)
        assert len(_cache["r1000"]) <= 65280
    return _cache["r1000"]


# ---- the well-formed fixtures --------------------------------------------------------------------------------------------------------

def _one(name, text, **kw):
    return Good(name, block(text, **kw), text, 1)


def _hand(name, stream, text):
    return Good(name, block(text, payload=stream), text, 1)


def good_fixtures():
    """-> [Good]: every one a BGZF file gzip.decompress reads as its text"""
    if "good" in _cache:
        return _cache["good"]
    g = []
    fq = records_1000()
    # compressor settings
    g.append(_one("level0_stored", fq, level=0))
    g.append(_one("z_fixed", fq, strategy=zlib.Z_FIXED))
    for lv in (1, 6, 9):
        g.append(_one("level%d" % lv, fq, level=lv))
    g.append(_one("z_huffman_only", fq, strategy=zlib.Z_HUFFMAN_ONLY))
    g.append(_one("z_rle", fq, strategy=zlib.Z_RLE))
    # stored blocks: length 0, and the longest a BGZF block holds (65536 - 26 header / trailer - 5 of the stored block)
    g.append(_hand("stored_len0", b"\x01\x00\x00\xff\xff", b""))
    big = bytes(np.random.default_rng(5).integers(0, 256, size=65505, dtype=np.uint8))
    g.append(_hand("stored_longest", b"\x01" + struct.pack("<HH", 65505, 65505 ^ 0xFFFF) + big, big))
    # sizes
    g.append(_one("isize_65536", b"ACGT" * 16384))
    for n in (1, 2, 3, 4):
        g.append(_one("text_%d_bytes" % n, b"@r1\n"[:n]))
    # several DEFLATE blocks in one BGZF block: full flushes leave empty stored blocks between dynamic ones, a fixed one ends it
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    parts = [fq[:9000], fq[9000:20000], fq[20000:20003], fq[20003:30000]]
    stream = b"".join(co.compress(p) + co.flush(zlib.Z_FULL_FLUSH) for p in parts[:-1]) + co.compress(parts[-1]) + co.flush()
    g.append(_hand("several_deflate_blocks", stream, fq[:30000]))
    # 15-bit codes: lengths 1, 2, ..., 14, 15, 15 over fifteen bytes and the end-of-block code; no distance code at all
    syms = list(b"ACGTNacgtn@+#IF")
    pairs = [(s, i + 1) for i, s in enumerate(syms[:14])] + [(syms[14], 15), (256, 15)]
    toks = [syms[i % 15] for i in range(400)] + [syms[14]] * 5 + [syms[13]] * 3
    w = Bits()
    dynamic_block(w, lens_of(pairs, 257), [0], toks)
    g.append(_hand("codes_of_15_bits_no_distance_code", w.done(), expand(toks)))
    # one distance code (a single code of length 1: incomplete, accepted)
    pairs = [(65, 2), (67, 2), (256, 3), (257, 3), (285, 2)]
    toks = [65, (3, 1), 67, (258, 1), 65, 67, (3, 1)]
    w = Bits()
    dynamic_block(w, lens_of(pairs, 286), [1], toks)
    g.append(_hand("one_distance_code", w.done(), expand(toks)))
    # a 16-repeat across the literal/distance boundary: 256, 257 and the eight distance codes all of length 3
    lit = lens_of([(65, 2), (67, 2), (71, 3), (84, 3), (256, 3), (257, 3)], 258)
    dst = [3] * 8
    seq = plain_cl_seq(lit[:257]) + [(16, 3)] + plain_cl_seq(dst[5:])  # 3 + 3 = 6 copies: 257 and distance codes 0 .. 4
    toks = [65, 67, 71, 84, (3, 4), (3, 1), (3, 7), 84, (3, 13)]
    w = Bits()
    dynamic_block(w, lit, dst, toks, seq)
    g.append(_hand("repeat16_across_boundary", w.done(), expand(toks)))
    # 17 and 18 at their longest: 138 zeros and 10 zeros in one go
    lit = lens_of([(65, 2), (67, 2), (71, 3), (84, 3), (256, 2)], 257)
    seq = [(18, 65 - 11)] + plain_cl_seq(lit[65:85]) + [(18, 127), (17, 7), (18, 23 - 11)] + [(2, 0)] + [(0, 0)]
    assert 65 + 20 + 138 + 10 + 23 + 1 == 257
    toks = [65, 67, 71, 84] * 9
    w = Bits()
    dynamic_block(w, lit, [0], toks, seq)
    g.append(_hand("repeat17_repeat18_longest", w.done(), expand(toks)))
    # hand-built fixed-Huffman streams
    toks = [81, (258, 1), 10]
    w = Bits()
    fixed_block(w, toks)
    g.append(_hand("length258_distance1", w.done(), expand(toks)))
    lead = [int(b) for b in np.random.default_rng(6).integers(33, 127, size=32768)]
    toks = lead + [(3, 32768), (258, 32768), (258, 1)]
    w = Bits()
    fixed_block(w, toks)
    g.append(_hand("length3_distance32768", w.done(), expand(toks)))
    toks = lead[:700] + [(9, 700), 65, (4, 710)]  # distance = position exactly, twice
    w = Bits()
    fixed_block(w, toks)
    g.append(_hand("distance_is_position", w.done(), expand(toks)))
    # every length code and every distance code once (the distance codes' base values, and their largest extra)
    toks = lead[:24600]
    for i in range(30):
        toks.append((LEN_BASE[i % 29], DIST_BASE[i]))
    for i in range(29):
        toks.append((LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1 if i < 28 else 258, min(32768, DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1)))
    w = Bits()
    fixed_block(w, toks)
    g.append(_hand("every_length_and_distance_code", w.done(), expand(toks)))
    # files
    g.append(Good("eof_block_alone", EOF_BLOCK, b"", 1))
    g.append(Good("isize0_block_in_the_middle", block(fq[:500]) + EOF_BLOCK + block(fq[500:900]) + EOF_BLOCK, fq[:900], 4))
    rng = np.random.default_rng(9)
    long_text = fastq_text(4500, 100, 12)
    pieces, at = [], 0
    for _ in range(300):
        n = int(rng.integers(10, 201))
        pieces.append(long_text[at:at + n])
        at += n
    g.append(Good("blocks_300_small", b"".join(block(p, level=int(rng.integers(0, 10))) for p in pieces), b"".join(pieces), 300))
    assert len(long_text) > 900000
    data = bgzf(long_text)
    g.append(Good("fastq_1mb_bgzip_shape", data, long_text, (len(long_text) + 65279) // 65280 + 1))
    assert len({f.name for f in g}) == len(g)
    _cache["good"] = g
    return g


# ---- the malformed fixtures ----------------------------------------------------------------------------------------------------------

def bad_fixtures():
    """-> [Bad]: reason / block are what mhx_bgzf_inflate must report; zlib_raises: gzip.decompress rejects the file (the others are
    valid gzip that is not BGZF)"""
    if "bad" in _cache:
        return _cache["bad"]
    R = REASONS
    fq = records_1000()
    ok = block(fq[:4000])
    b = []

    def in_file(name, bad_block, reason, zlib_raises=True):
        # the bad block second of three, so that the index is not 0
        b.append(Bad(name, ok + bad_block + ok + EOF_BLOCK, reason, 1, zlib_raises))

    text = fq[4000:9000]
    in_file("payload_cut_by_one_byte", block(text, payload=deflate(text)[:-1]), R["PAYLOAD_END"])
    in_file("btype3", block(b"", payload=b"\x07"), R["BTYPE"])
    in_file("nlen_wrong", block(b"hello", payload=b"\x01\x05\x00\x00\x00hello"), R["STORED_LEN"])
    w = Bits()
    dynamic_block(w, lens_of([(65, 1), (67, 1), (256, 1)], 257), [0], [65, 67])
    in_file("oversubscribed_literal_code", block(b"AC", payload=w.done()), R["CODE_OVER"])
    w = Bits()
    fixed_block(w, [65, (3, 2)])
    in_file("distance_one_past_the_start", block(b"AAAA", payload=w.done()), R["DIST_FAR"])
    in_file("stream_yields_isize_plus_1", block(text[:-1], payload=deflate(text)), R["OUT_OVER"])
    in_file("stream_yields_isize_minus_1", block(text + b"\n", payload=deflate(text)), R["OUT_SHORT"])
    in_file("wrong_crc", block(text, crc=zlib.crc32(text) ^ 0x00100000), R["CRC"])
    in_file("wrong_isize", block(text, isize=len(text) + 10), R["OUT_SHORT"])
    in_file("plain_gzip_member_between", gzip.compress(text, mtime=0), R["FLG"], zlib_raises=False)
    b.append(Bad("trailing_junk", ok + EOF_BLOCK + b"junk", R["TRAILING"], 2, True))
    assert len({f.name for f in b}) == len(b)
    _cache["bad"] = b
    return b
