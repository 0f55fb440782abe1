"""GPU: the FASTA / FASTQ parser (csrc/fastx.hip behind mhx_fastx_to_records, with the scans of csrc/scan.hip) at line, chunk,
block and scan-tile edges, against the reader model of tests/fastx_model.py (which tests/test_fastx_model.py pins to the
reference binary).  The rule for every text and every pair of mate texts:
  - status 0: the records and n_reads / n_bases / n_words / max_len are exactly the model's;
  - a text the parser's contract covers (fastx_model.plain) must come back with status 0, so declining is no way to pass.
Every comparison is equality of integers and bytes."""
import numpy as np
import pytest

import fastx_cases as fc
import fastx_model as fm

pytestmark = pytest.mark.gpu

_expected = {}


def expected(name, text1, text2=None):
    if name not in _expected:
        _expected[name] = fm.expected(text1, text2) + (len(fm.records(text1)), None if text2 is None else len(fm.records(text2)))
    return _expected[name]


def judge(engine, name, text1, text2=None, want=None):
    """one call, judged by the rule above; -> status"""
    words, n_reads, n_bases, max_len, n1, n2 = want or expected(name, text1, text2)
    r, rec = engine.fastx_to_records(text1, text2)
    assert r.status in (0, 1), name
    # mates of unequal count may go to the sequential parser, which stops when either file ends
    if fm.plain(text1) and (text2 is None or (fm.plain(text2) and n1 == n2)):
        assert r.status == 0, "%s: inside the parser's contract, yet declined" % name
    if r.status == 0:
        assert (r.n_reads, r.n_bases, r.n_words, r.max_len) == (n_reads, n_bases, words.size, max_len), name
        assert rec.dtype == np.uint32 and np.array_equal(rec, words), name
    return r.status


def test_header_char_as_the_last_byte(engine):
    """the reference's reader returns no record for a '>' with nothing behind it: 1, 0, 2, 2 records"""
    for k, (text, n_rec) in enumerate(((b">a\nACGT\n>", 1), (b">", 0), (b">a\nACGT\n>\n", 2), (b">a\nACGT\n>b", 2), (b">\n", 1), (b"> \n", 1))):
        assert expected("last_byte_%d" % k, text)[1] == n_rec
        judge(engine, "last_byte_%d" % k, text)


def test_fixed_fasta_edges(engine):
    for name, text in fc.fixed_fasta():
        judge(engine, name, text)


def test_fixed_fastq_edges(engine):
    for name, text in fc.fixed_fastq():
        assert fm.plain(text), name
        assert judge(engine, name, text) == 0


def test_shapes_outside_the_contract_are_declined_or_right(engine):
    for name, text in fc.declined_fastq():
        assert not fm.plain(text), name
        judge(engine, name, text)


def test_newlines_at_chunk_block_and_tile_boundaries(engine):
    for name, text in fc.boundary_texts():
        assert fm.plain(text), name
        assert judge(engine, name, text) == 0


def test_scan_of_more_than_1024_tiles_of_lines(engine):
    """one record of CARRY_LINES one-base lines: the top-level scan of the line scans goes round its carry loop"""
    text, rec = fc.carry_text_and_record()
    assert fm.plain(text)
    assert judge(engine, "carry", text, want=(rec, 1, fc.CARRY_LINES, fc.CARRY_LINES, 1, None)) == 0


def test_paired_texts(engine):
    for name, t1, t2 in fc.fixed_pairs():
        st = judge(engine, name, t1, t2)
        if name in ("pe_fa_fa", "pe_fq_fq", "pe_fa_fq", "pe_fq_fa", "pe_300_records", "pe_both_empty"):
            assert st == 0, name


def test_seeded_random_plain_texts(engine):
    for name, text in fc.random_texts():
        assert fm.plain(text), name
        assert judge(engine, name, text) == 0


def test_seeded_random_pairs(engine):
    for name, t1, t2 in fc.random_pairs():
        assert fm.plain(t1) and fm.plain(t2), name
        assert judge(engine, name, t1, t2) == 0


def test_workspaces_reused_across_calls(engine):
    """the workspaces of one context are kept between calls and never zeroed: large, declined, small, empty, large again"""
    big = fc.over_2048_chunks()
    declined = dict(fc.declined_fastq())["fq_short_quality_not_last"]
    for name, text in (("fa_over_2048_chunks", big), ("fq_short_quality_not_last", declined), ("fa_three_records", fc.THREE_RECORDS), ("empty", b""),
                       ("one_record", b">a\nACGT\n"), ("fa_over_2048_chunks", big)):
        assert judge(engine, name, text) == 0 or text is declined, name
    for name, text in reversed(fc.fixed_fasta() + fc.fixed_fastq() + fc.declined_fastq()):
        judge(engine, name, text)
