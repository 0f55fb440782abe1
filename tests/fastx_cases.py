"""FASTA / FASTQ texts at the edges of the GPU parser (csrc/fastx.hip): line, 256-byte chunk, 64 KiB block and 2048-item scan
tile boundaries, record lengths around the 16-base word and the 64-lane wave, N placement, and the shapes the parser
declines.  Shared by tests/test_fastx_model.py (model = reference binary) and tests/test_gpu_fastx_edges.py (kernels = model).
Every text is bytes over 0x20..0x7E, tab and newline; '\\r' only in the CRLF cases."""
import numpy as np

LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
BOUNDARIES = (256, 512, 65536, 65792)  # chunk, two chunks, one block of the newline kernels, a block and a chunk
CARRY_LINES = 2097153 + 2048           # more than 1024 scan tiles of lines
THREE_RECORDS = b">a\nACGTNNACGT\n>b\nnnnn\n>c\nacgtacgtacgtacgtacgt\n"


def bases(L, seed):
    """L bytes of ACGT"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=L)].tobytes()


def wrap(s, width):
    return b"\n".join(s[i:i + width] for i in range(0, len(s), width))


def fasta(seqs, width=None, name=b"r"):
    return b"".join(b">%s%d\n%s\n" % (name, i, wrap(s, width) if width else s) for i, s in enumerate(seqs))


def fastq(seqs, plus=b"+", qual=None):
    return b"".join(b"@q%d\n%s\n%s\n%s\n" % (i, s, plus, qual[i] if qual else b"I" * len(s)) for i, s in enumerate(seqs))


def n_placement_seqs():
    out = []
    for L in (1, 16, 17, 33):
        s = bytearray(bases(L, 100 + L))
        for at in (0, 15, 16, L - 1):
            if at < L:
                t = bytearray(s)
                t[at] = ord("N")
                out.append(bytes(t))
        out += [b"N" * L, b"n" * L]
    out += [b"NANNN", b"NNACGTNNACGT"]
    # N-free stretches that end exactly at a word boundary of the record: 16 and 32 kept bases
    out += [bases(16, 7) + b"N" + bases(5, 8), b"N" + bases(32, 9) + b"n" + bases(40, 10), bases(32, 11) + b"N"]
    return out


def fixed_fasta():
    """-> [(name, text)]"""
    by_len = [bases(L, L) for L in LENGTHS]
    long_rec = bases(70000, 70000)
    t = [("fa_lengths", fasta(by_len)), ("fa_lengths_wrap16", fasta(by_len, 16)), ("fa_long_one_line", b">long\n" + long_rec + b"\n")]
    t += [("fa_long_wrap%d" % w, b">long\n" + wrap(long_rec, w) + b"\n") for w in (1, 60, 63, 64, 65)]
    t += [
        ("fa_blank_lines", b">a\n\nACGT\n\n\nTTGCA\n\n>b\n\n\n>c\nGG\n\nC\n"),
        ("fa_header_only_records", b">a\n>b\n>c\n>d\nACGT\n>e\n>f\n"),
        ("fa_last_line_no_newline", b">a\nACGT\n>b\nTTGCAAC"),
        ("fa_header_last_no_newline", b">a\nACGT\n>b"),
        ("fa_trailing_blank_lines", b">a\nACGT\n>b\nTTG\n\n\n"),
        ("fa_bare_header_at_eof", b">a\nACGT\n>"),
        ("fa_only_header_char", b">"),
        ("fa_only_header_line", b">\n"),
        ("fa_header_of_one_space", b"> \n"),
        ("fa_header_char_then_newline_last", b">a\nACGT\n>\n"),
        ("fa_header_with_tab", b">a\tb c\nACGT\n>\tx\nGGT\n"),
        ("fa_header_with_comment", b">a some comment > with @ and + signs\nACGT\n>b  \nTT\n"),
        ("fa_lines_led_by_blank", b">a\n ACGT\n\tCGT\n>b\n  \nT\n"),
        ("fa_lead_chars_mid_line", b">a\nAC>GT\nC+GT@A\nG@\n>b\nT>\n"),
        ("fa_lower_case", b">a\nacgtnacgt\n>b\nAcGtAcGtAcGtAcGtAcGt\n"),
        ("fa_other_letters", b">a\nACGTRYKMACGT\n>b\nrykmRYKMrykmRYKMrykm\n"),
        ("fa_n_placement", fasta(n_placement_seqs())),
        ("fa_n_placement_wrap5", fasta(n_placement_seqs(), 5)),
        ("fa_three_records", THREE_RECORDS),
        ("empty", b""),
    ]
    return t


def fixed_fastq():
    """four-line FASTQ the GPU parser must take -> [(name, text)]"""
    by_len = [bases(L, 300 + L) for L in LENGTHS]
    t = [
        ("fq_lengths", fastq(by_len)),
        ("fq_quality_led_by_at_plus_gt", fastq([b"ACGT", b"TTGCA", b"GGC", b"A"], qual=[b"@III", b"+IIII", b">II", b"@"])),
        ("fq_plus_name_lines", fastq(by_len[:6], plus=b"+q some text @ > +")),
        ("fq_last_quality_no_newline", fastq(by_len[:5])[:-1]),
        ("fq_sequence_led_by_n", fastq([b"NACGT", b"nnACGTNAC", b"N", b"ACGT"])),
        ("fq_at_mid_sequence", fastq([b"AC@GT", b"A>C+G@", b"ACGT"])),
        ("fq_n_placement", fastq(n_placement_seqs())),
        ("fq_header_only_at", b"@\nACGT\n+\nIIII\n@ \nTT\n+\n@@\n"),
    ]
    return t


def declined_fastq():
    """shapes the GPU parser may decline (status 1) -> [(name, text)]"""
    good = fastq([b"ACGT", b"TTGCA"])
    return [
        ("fq_multi_line", b"@a\nACGT\nTTGC\n+\nIIII\nIIII\n@b\nAC\n+\nII\n"),
        ("fq_empty_sequence", b"@a\n\n+\n\n@b\nAC\n+\nII\n"),
        ("fq_short_quality", b"@a\nACGTACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n"),
        ("fq_short_quality_not_last", good + b"@bad\nACGTACGT\n+\nIIII\n" + good),
        ("fq_line_count_not_4k", good + b"@c\nACGT\n+\n"),
        ("fq_four_trailing_blank_lines", good + b"\n\n\n\n"),
        ("fq_fasta_header_among", good + b">x\nACGT\n" + good),
        ("fq_sequence_led_by_plus", b"@a\n+CGT\n+\nIIII\n@b\nAC\n+\nII\n"),
        ("fq_crlf", good.replace(b"\n", b"\r\n")),
        ("fa_crlf", b">a\r\nACGT\r\n>b\r\nT\r\n\r\nGG\r\n"),
        ("fa_crlf_blank_line_first", b">a\r\n\r\nAC\r\n>b\r\n\r\n"),
        ("fq_junk_before_header",b"junk line\n" + good),
        ("fa_junk_before_header", b"junk > line\nACGT\n>b\nTT\n"),
        ("fa_plus_led_line", b">a\nACGT\n+\nIIII\n>b\nTT\n"),
        ("fa_at_led_line", b">a\nACGT\n@b\nTT\n"),
        ("fq_bare_header_at_eof", good + b"@"),
    ]


def _mixed_records(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.array(LENGTHS + (0, 2, 100)), size=n)
    return [bases(int(L), seed * 100003 + i) for i, L in enumerate(lens)]


def _body(fmt, seqs):
    if fmt == "fa":
        return fasta(seqs, name=b"m")
    return fastq([s or b"A" for s in seqs])


def _lead(fmt):
    return b">" if fmt == "fa" else b"@"


def newline_at(fmt, off, which):
    """a text of records whose chosen newline sits at byte offset `off`: which = 'hdr' (the newline that ends a padded
    header line) or 'seq' (the one that ends the sequence line after it); more records follow"""
    seqs = _mixed_records(off // 40 + 4, off + (which == "seq"))  # a record averages some 90 bytes: twice what is needed
    body = b""
    k = 0
    while k < len(seqs) and len(body) + len(_body(fmt, seqs[k:k + 1])) < off - 150:
        body += _body(fmt, seqs[k:k + 1])
        k += 1
    s = bases(33, off)
    room = off - len(body) - (len(s) + 1 if which == "seq" else 0)  # bytes of the padded header line before its newline
    assert room >= 1
    text = body + _lead(fmt) + b"p" * (room - 1) + b"\n" + s + b"\n" + (b"+\n%s\n" % (b"I" * len(s)) if fmt == "fq" else b"")
    text += _body(fmt, [bases(17, 1), bases(64, 2), bases(1, 3)])
    assert text[off] == 0x0A and (text[off - len(s) - 1] == 0x0A if which == "seq" else text[off + len(s) + 1] == 0x0A)
    return text


def total_length(fmt, n, final_newline):
    """a text of records of exactly n bytes"""
    body = _body(fmt, [bases(L, n + L) for L in (1, 16, 17, 33, 64, 65)])
    s = bases(20, n)
    tail = s + b"\n" + (b"+\n%s\n" % (b"I" * len(s)) if fmt == "fq" else b"")
    if not final_newline:
        tail = tail[:-1]
    pad = n - len(body) - len(tail) - 2
    assert pad >= 0
    text = body + _lead(fmt) + b"p" * pad + b"\n" + tail
    assert len(text) == n
    return text


def boundary_texts():
    """-> [(name, text)], all plain"""
    t = []
    for fmt in ("fa", "fq"):
        for B in BOUNDARIES:
            for off in (B - 1, B):
                for which in ("hdr", "seq"):
                    t.append(("%s_newline_%s_at_%d" % (fmt, which, off), newline_at(fmt, off, which)))
        for n in (256 * 5 - 1, 256 * 5, 256 * 5 + 1):
            for nl in (True, False):
                t.append(("%s_total_%d_%s" % (fmt, n, "nl" if nl else "no_nl"), total_length(fmt, n, nl)))
        many = _mixed_records(2100, 21 if fmt == "fa" else 22)
        t.append(("%s_2100_records" % fmt, fasta(many, 60) if fmt == "fa" else _body(fmt, many)))
        t.append(("%s_300_records" % fmt, _body(fmt, _mixed_records(300, 23))))
    t.append(("fa_over_2048_chunks", over_2048_chunks()))
    return t


_cache = {}


def over_2048_chunks():
    """just over 2048 * 256 bytes of FASTA: the scan over the per-chunk newline counts takes a second tile"""
    if "big" not in _cache:
        seqs = _mixed_records(7000, 31)
        text = fasta(seqs, 70)
        assert len(text) > 2048 * 256 + 300
        cut = text.rfind(b"\n>", 0, 2048 * 256 + 300) + 1  # whole records only
        assert cut > 2048 * 256
        _cache["big"] = text[:cut]
    return _cache["big"]


def carry_text_and_record():
    """one header, then CARRY_LINES one-base lines: one record.  -> (text, its record words), the record in closed form"""
    if "carry" not in _cache:
        codes = np.random.default_rng(5).integers(0, 4, size=CARRY_LINES).astype(np.uint8)
        lines = np.empty((CARRY_LINES, 2), dtype=np.uint8)
        lines[:, 0] = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
        lines[:, 1] = 0x0A
        text = b">carry\n" + lines.tobytes()
        padded = np.zeros((CARRY_LINES + 15) // 16 * 16, dtype=np.uint32)
        padded[:CARRY_LINES] = codes
        body = np.bitwise_or.reduce(padded.reshape(-1, 16) << np.arange(30, -2, -2, dtype=np.uint32), axis=1).astype(np.uint32)
        _cache["carry"] = (text, np.concatenate([np.array([CARRY_LINES], dtype=np.uint32), body]))
    return _cache["carry"]


def fixed_pairs():
    """-> [(name, text1, text2)]"""
    a = [bases(L, 500 + L) for L in (1, 16, 17, 33, 64, 100)]
    b = [bases(L, 600 + L) for L in (100, 65, 32, 17, 15, 1)]
    a[2] = b"NNNN"   # mates that trim to nothing, on either side and on both
    b[4] = b"n"
    a[5] = b"NN"
    b[5] = b"N" * 17
    return [
        ("pe_fa_fa", fasta(a), fasta(b, 20)),
        ("pe_fq_fq", fastq(a), fastq(b)),
        ("pe_fa_fq", fasta(a, 7), fastq(b)),
        ("pe_fq_fa", fastq(a), fasta(b)),
        ("pe_300_records", fasta(_mixed_records(300, 41)), _body("fq", _mixed_records(300, 42))),
        ("pe_unequal_first_longer", fasta(a), fasta(b[:4])),
        ("pe_unequal_second_longer", fastq(a[:2]), fastq(b)),
        ("pe_one_empty", fasta(a), b""),
        ("pe_both_empty", b"", b""),
        # a malformed record in one mate file: the build reads on behind it, and the other file's record of that turn is lost
        ("pe_malformed_first", fastq(a[:2]) + b"@bad\nACGTACGT\n+\nIIII\n" + fastq(a[2:]), fasta(b)),
        ("pe_malformed_second", fasta(a), fastq(b[:3]) + b"@bad\nACGTACGT\n+\nIIII\n" + fastq(b[3:])),
    ]


# ---- seeded random plain texts -------------------------------------------------------------------------------------------

def _printable(rng, n, lo=33):
    return rng.integers(lo, 127, size=n).astype(np.uint8).tobytes()


def _random_seq(rng, L):
    s = bytearray(b"ACGT"[i] for i in rng.integers(0, 4, size=L))
    if L and rng.random() < 0.3:
        s = bytearray(bytes(s).lower())
    for _ in range(int(rng.integers(0, 3))):  # N runs at drawn positions
        if L:
            at, run = int(rng.integers(0, L)), int(rng.integers(1, 5))
            s[at:at + run] = (b"N" if rng.random() < 0.7 else b"n") * len(s[at:at + run])
    if L and rng.random() < 0.3:  # stray letters, any printable byte, blank or tab
        for at in rng.integers(0, L, size=int(rng.integers(1, 4))):
            s[int(at)] = int(rng.choice(np.frombuffer(_printable(rng, 6, 32) + b"\t", dtype=np.uint8)))
    return s


def _random_header(rng, lead):
    h = lead + _printable(rng, int(rng.integers(0, 8)))
    if rng.random() < 0.4:
        h += (b" " if rng.random() < 0.7 else b"\t") + _printable(rng, int(rng.integers(0, 12)), 32)
    return h


def _random_length(rng, lo):
    return max(lo, int(rng.choice(np.array(LENGTHS))) + int(rng.integers(-1, 2)))


def random_fasta(seed, n_rec=None):
    rng = np.random.default_rng([seed, 1])
    n_rec = n_rec or int(rng.integers(1, 41))
    width = None if rng.random() < 0.4 else int(rng.choice(np.array([1, 15, 16, 17, 60, 63, 64, 65])))
    lines = []
    for _ in range(n_rec):
        lines.append(_random_header(rng, b">"))
        s = _random_seq(rng, _random_length(rng, 0))
        w = width if width != 1 or len(s) < 40 else 60
        for i in range(0, len(s), w or max(1, len(s))):
            line = s[i:i + w] if w else s
            if line[:1] in (b">", b"+", b"@"):  # would be a header, or FASTQ
                line[0] = ord("A")
            lines.append(bytes(line))
            if rng.random() < 0.05:
                lines.append(b"")
    text = b"\n".join(lines)
    if rng.random() < 0.7 or lines[-1] == b">":
        text += b"\n" * (1 if rng.random() < 0.8 else 3)
    return text


def random_fastq(seed, n_rec=None):
    rng = np.random.default_rng([seed, 2])
    n_rec = n_rec or int(rng.integers(1, 41))
    lines = []
    for _ in range(n_rec):
        s = _random_seq(rng, _random_length(rng, 1))
        if s[:1] in (b">", b"+", b"@"):
            s[0] = ord("C")
        lines += [_random_header(rng, b"@"), bytes(s), b"+" + (_printable(rng, int(rng.integers(0, 6)), 32) if rng.random() < 0.3 else b""),
                  _printable(rng, len(s))]
    return b"\n".join(lines) + (b"\n" if rng.random() < 0.7 else b"")


RANDOM_SEEDS = tuple(range(1000, 1040))


def random_texts():
    """-> [(name, text)]: 40 FASTA and 40 FASTQ, plain by construction"""
    return [("rnd_fa_%d" % s, random_fasta(s)) for s in RANDOM_SEEDS] + [("rnd_fq_%d" % s, random_fastq(s)) for s in RANDOM_SEEDS]


def random_pairs():
    """-> [(name, text1, text2)]: 20 pairs of equal record count"""
    out = []
    for s in range(2000, 2020):
        n = 1 + s % 13
        g1, g2 = ((random_fasta, random_fasta), (random_fastq, random_fastq), (random_fasta, random_fastq), (random_fastq, random_fasta))[s % 4]
        out.append(("rnd_pe_%d" % s, g1(s, n), g2(s + 500, n)))
    return out


def plain_singles():
    """every single text that csrc/fastx.hip has to parse itself"""
    return [(n, t) for n, t in fixed_fasta() if n not in ("fa_bare_header_at_eof", "fa_only_header_char")] + fixed_fastq() + boundary_texts() + random_texts()


def all_singles():
    return fixed_fasta() + fixed_fastq() + declined_fastq() + boundary_texts() + random_texts()


def all_pairs():
    return fixed_pairs() + random_pairs()
