"""A plain model of the read library's reader: FASTA / FASTQ text -> sequences -> the record stream of the .bin file.

`records` says which sequences a text holds, record by record, the way the reference's line reader finds them; `pack`
says what the library file holds for them (N-trimming, the 2-bit codes, the length word); `plain` says which texts the GPU
parser (csrc/fastx.hip) promises to take itself instead of handing them to the sequential parser.  tests/test_fastx_model.py
pins all three to the reference binary before any kernel is judged by them."""
import numpy as np

_WS = b" \t\n\v\f\r"
_LEADS = b">+@"


def _next_header(text, i):
    """index of the first '>' or '@' at or after i, or -1"""
    a, b = text.find(b">", i), text.find(b"@", i)
    if a < 0:
        return b
    return a if b < 0 else min(a, b)


def _append_line(acc, text, i):
    """the rest of the line at i goes onto acc; a '\\r' goes only when it ends an accumulated string longer than 1.
    -> index after the line's newline"""
    e = text.find(b"\n", i)
    if e < 0:
        e = len(text)
    acc += text[i:e]
    if len(acc) > 1 and acc[-1] == 0x0D:
        del acc[-1]
    return min(e + 1, len(text))


class Reader:
    """One text, read record by record.  next() -> the sequence (bytes, untrimmed) of the next record, or None: the end of
    the text, or a malformed FASTQ record.  After a malformed record a further next() reads on from where that one stopped."""

    def __init__(self, text):
        self.text = bytes(text)
        self.i = 0
        self.pending = False  # the header char of the next record has been consumed already
        self.at_end = False

    def _end(self):
        self.at_end = True
        return None

    def next(self):
        text, n = self.text, len(self.text)
        if self.at_end:
            return None
        if not self.pending:
            h = _next_header(text, self.i)
            if h < 0:
                return self._end()
            self.i = h + 1
        self.pending = False
        i = self.i
        if i >= n:  # a header char as the very last byte: nothing to read a name from
            return self._end()
        # the name runs to the first whitespace; unless that is the newline, the rest of the line is a comment
        e = i
        while e < n and text[e] not in _WS:
            e += 1
        i = min(e + 1, n)
        if e < n and text[e] != 0x0A:
            i = _append_line(bytearray(), text, i)
        # sequence lines, until a line begins with '>', '+' or '@'
        seq = bytearray()
        lead = None
        while i < n:
            ch = text[i]
            i += 1
            if ch in _LEADS:
                lead = ch
                break
            if ch == 0x0A:  # an empty line
                continue
            seq.append(ch)
            i = _append_line(seq, text, i)
        self.i = i
        if lead != 0x2B:  # FASTA, or the last record of the text
            self.pending = lead is not None
            self.at_end = lead is None
            return bytes(seq)
        # FASTQ: the rest of the '+' line is ignored, then quality lines until they cover the sequence
        e = text.find(b"\n", i)
        if e < 0:  # no quality line at all
            return self._end()
        i = e + 1
        qual = bytearray()
        while i < n:
            i = _append_line(qual, text, i)
            if len(qual) >= len(seq):
                break
        self.i = i
        return bytes(seq) if len(qual) == len(seq) else None


def _until_nothing_comes(read_some):
    """The library is built batch by batch: a batch ends where the reader returns nothing (the end of the text or a
    malformed record), the next one reads on, and the build ends with the first batch that is empty.  So a malformed
    record is skipped, with whatever its over-long quality read swallowed, unless it is the first record or follows
    another malformed one directly.  (The reference also ends a batch after 2^22 records or 2^28 bases: no text here
    gets there.)"""
    out = []
    while True:
        before = len(out)
        read_some(out)
        if len(out) == before:
            return out


def records(text):
    """the sequences of the records a library of this text holds, in order"""
    r = Reader(text)

    def batch(out):
        while True:
            s = r.next()
            if s is None:
                return
            out.append(s)
    return _until_nothing_comes(batch)


def paired_records(text1, text2):
    """the sequences of a library of two mate texts, alternating; both texts are read in step, a pair counts when both
    readers return a record, and a batch ends when either returns nothing"""
    a, b = Reader(text1), Reader(text2)

    def batch(out):
        while True:
            x, y = a.next(), b.next()
            if x is None or y is None:
                return
            out += [x, y]
    return _until_nothing_comes(batch)


_CODE = np.zeros(256, dtype=np.uint32)
for _chars, _v in ((b"Cc", 1), (b"GgNn", 2), (b"Tt", 3)):
    for _c in _chars:
        _CODE[_c] = _v


def trim_n(seq):
    """the first maximal stretch without N/n (empty when there is none)"""
    b = 0
    while b < len(seq) and seq[b] in b"Nn":
        b += 1
    e = b
    while e < len(seq) and seq[e] not in b"Nn":
        e += 1
    return seq[b:e]


def pack_one(seq):
    """one sequence -> its record words: the length, then 16 bases per word, the first base in the top two bits"""
    s = trim_n(bytes(seq)) or b"A"
    L = len(s)
    codes = np.zeros((L + 15) // 16 * 16, dtype=np.uint32)
    codes[:L] = _CODE[np.frombuffer(s, dtype=np.uint8)]
    shifts = np.arange(30, -2, -2, dtype=np.uint32)
    body = np.bitwise_or.reduce(codes.reshape(-1, 16) << shifts, axis=1).astype(np.uint32)
    return np.concatenate([np.array([L], dtype=np.uint32), body]), L


def pack(seqs, interleave_with=None):
    """-> (uint32 words, n_reads, n_bases, max_len); interleave_with: the mates, alternated record by record up to the
    end of the shorter list"""
    if interleave_with is not None:
        seqs = [s for pair in zip(seqs, interleave_with) for s in pair]
    parts, n_bases, max_len = [], 0, 0
    for s in seqs:
        w, L = pack_one(s)
        parts.append(w)
        n_bases += L
        max_len = max(max_len, L)
    words = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return words, len(seqs), n_bases, max_len


def expected(text1, text2=None):
    """what a library of this text (these two mate texts) holds"""
    return pack(records(text1) if text2 is None else paired_records(text1, text2))


def plain(text):
    """True: csrc/fastx.hip must parse this text itself (status 0).  The contract at the top of that file."""
    text = bytes(text)
    if b"\r" in text:
        return False
    if not text:
        return True
    if text[0] not in b">@":
        return False
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    if text[0] == 0x3E:
        if any(l[:1] in (b"+", b"@") for l in lines):
            return False
        # a bare '>' as the last byte, at a line start: the reader returns no record for it; the GPU parser declines
        return not (text.endswith(b">") and (len(text) == 1 or text[-2] == 0x0A))
    if len(lines) % 4:
        return False
    for k in range(0, len(lines), 4):
        h, s, p, q = lines[k:k + 4]
        if h[:1] != b"@" or p[:1] != b"+" or not s or s[:1] in (b">", b"+", b"@") or len(q) != len(s):
            return False
    return True
