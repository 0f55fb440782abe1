"""CPU: the BGZF scan (megahit_amd/csrc/bgzf_scan.h) and the one-lane host build of the inflate core the GPU kernel runs
(megahit_amd/csrc/inflate_core.h), driven by a small C++ program built here with g++ under AddressSanitizer and UBSan (no GPU, no libmhx,
no HIP header): tests/host/bgzf_check.cpp.  It inflates every fixture of tests/bgzf_util.py and compares text, status, reason and block;
the malformed fixtures show the core's bounds rules to hold on exactly the inputs the GPU tests send, and 360 blocks with one payload
bit flipped must be inflated exactly when zlib inflates them."""
import gzip
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "bgzf_check.cpp")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def extra_scan_cases():
    """members the scan must decline that no zlib-made file shows -> [Bad]"""
    R = bz.REASONS
    ok = bz.block(b"@r\nACGT\n+\nIIII\n")
    no_bc = bytearray(ok)
    no_bc[12:14] = b"XY"
    other_flg = bytearray(ok)
    other_flg[3] = 0x0C
    short = bytearray(bz.EOF_BLOCK)
    short[16:18] = (24).to_bytes(2, "little")  # BSIZE + 1 = 25
    big_isize = bytearray(ok)
    big_isize[-4:] = (65537).to_bytes(4, "little")
    return [
        bz.Bad("scan_no_bc_field", ok + bytes(no_bc), R["NO_BC"], 1, False),
        bz.Bad("scan_other_flg", ok + bytes(other_flg), R["FLG"], 1, False),
        bz.Bad("scan_isize_above_65536", bytes(big_isize), R["ISIZE"], 0, True),
        bz.Bad("scan_block_shorter_than_26", ok + bytes(short), R["SHORT_BLOCK"], 1, True),
        bz.Bad("scan_block_past_eof", ok + ok[:-3], R["PAST_EOF"], 1, True),
        bz.Bad("scan_not_gzip", ok + b"\0" * 40, R["NOT_GZIP"], 1, True),
    ]


def mutated_cases():
    """single-block files with one payload byte changed: inflated exactly when zlib inflates them -> [(name, data, text or None)]"""
    rng = np.random.default_rng(77)
    fq = bz.records_1000()[:6000]
    out = []
    for kind, src in (("dyn", bz.block(fq)), ("fix", bz.block(fq, strategy=zlib.Z_FIXED)), ("l1", bz.block(fq[:700], level=1))):
        for i in range(120):
            data = bytearray(src)
            at = int(rng.integers(18, len(src) - 8)) if i >= 40 else 18 + i  # the first 40: the block header and the code lengths
            data[at] ^= 1 << int(rng.integers(0, 8))
            try:
                text = gzip.decompress(bytes(data))
            except (zlib.error, gzip.BadGzipFile, EOFError):
                text = None
            out.append(("mut_%s_%d" % (kind, i), bytes(data), text))
    return out


def test_scan_and_one_lane_inflate_under_sanitizers(tmp_path):
    d = str(tmp_path)
    exe = os.path.join(d, "bgzf_check")
    subprocess.run(GXX + ["-o", exe], check=True)
    lines = []
    for fx in bz.good_fixtures():
        open(os.path.join(d, fx.name + ".gz"), "wb").write(fx.data)
        open(os.path.join(d, fx.name + ".txt"), "wb").write(fx.text)
        lines.append("%s 0 0 0" % fx.name)
    bad = bz.bad_fixtures() + extra_scan_cases()
    for fx in bad:
        open(os.path.join(d, fx.name + ".gz"), "wb").write(fx.data)
        lines.append("%s 2 %d %d" % (fx.name, fx.reason, fx.block))
    for name, data, text in mutated_cases():
        open(os.path.join(d, name + ".gz"), "wb").write(data)
        if text is not None:
            open(os.path.join(d, name + ".txt"), "wb").write(text)
        lines.append("%s %d 255 0" % (name, 0 if text is not None else 2))
    open(os.path.join(d, "cases.txt"), "w").write("\n".join(lines) + "\n")
    p = subprocess.run([exe, d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok %d" % len(lines), p.stderr
