"""CPU: the BGZF fixtures of tests/bgzf_util.py against zlib itself, so that the GPU tests (tests/test_gpu_bgzf.py) and the host check
(tests/test_host_bgzf.py) are not held to the helper's bugs: every well-formed fixture is a file gzip.decompress reads as its text,
every malformed one is a file zlib rejects (or, where it is valid gzip that is not BGZF, one whose members show it)."""
import gzip
import os
import re
import struct
import zlib

import pytest

import bgzf_util as bz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def members(data):
    """walk BGZF members by their BSIZE -> [(payload, crc, isize)]"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 10:o + 16] == b"\x06\x00BC\x02\x00"
        total = struct.unpack_from("<H", data, o + 16)[0] + 1
        out.append((data[o + 18:o + total - 8],) + struct.unpack_from("<II", data, o + total - 8))
        o += total
    assert o == len(data)
    return out


@pytest.mark.parametrize("fx", bz.good_fixtures(), ids=lambda f: f.name)
def test_well_formed_fixture_is_gzip_of_its_text(fx):
    assert gzip.decompress(fx.data) == fx.text
    ms = members(fx.data)
    assert len(ms) == fx.n_blocks
    text = b""
    for payload, crc, isize in ms:
        t = zlib.decompress(payload, -15)
        assert len(t) == isize <= 65536 and zlib.crc32(t) == crc
        text += t
    assert text == fx.text


@pytest.mark.parametrize("fx", bz.bad_fixtures(), ids=lambda f: f.name)
def test_malformed_fixture_is_rejected_by_zlib_or_is_not_bgzf(fx):
    if fx.zlib_raises:
        with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
            gzip.decompress(fx.data)
    else:
        gzip.decompress(fx.data)  # valid gzip ...
        with pytest.raises(AssertionError):  # ... with a member that is not a BGZF block
            members(fx.data)


def test_the_eof_block_is_the_standard_marker():
    assert bz.EOF_BLOCK == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000") and len(bz.EOF_BLOCK) == 28


def test_hand_built_streams_reach_what_zlib_never_emits():
    by_name = {f.name: f for f in bz.good_fixtures()}
    far = members(by_name["length3_distance32768"].data)[0][0]
    assert zlib.decompress(far, -15) == by_name["length3_distance32768"].text
    assert by_name["length3_distance32768"].text[32768:32771] == by_name["length3_distance32768"].text[:3]
    assert len(by_name["isize_65536"].data) < 200 and len(by_name["isize_65536"].text) == 65536
    assert len(members(by_name["stored_longest"].data)[0][0]) + 26 == 65536
    assert len(by_name["blocks_300_small"].text) > 10 * 300 and by_name["blocks_300_small"].n_blocks == 300
    assert all(isize <= 65280 for _, _, isize in members(by_name["fastq_1mb_bgzip_shape"].data))


def test_reason_codes_are_the_headers():
    with open(os.path.join(ROOT, "include", "mhx.h")) as fh:
        got = {k: int(v) for k, v in re.findall(r"\bMHX_BGZF_([A-Z_]+) = (\d+)", fh.read())}
    assert got == bz.REASONS
