"""GPU: BGZF read files inflated on the device (csrc/inflate.hip behind mhx_bgzf_inflate and mhx_fastx_bgzf_to_records, the opt-in
MHX_BUILDLIB_BGZF=1 route of `mhx_core buildlib`).  Every expectation is zlib's (tests/bgzf_util.py, held to zlib by
tests/test_bgzf_fixtures.py) or the existing route's on the text zlib inflates:
  - a well-formed fixture comes back status 0 with zlib's text, byte for byte: declining what zlib accepts is a failure;
  - a malformed one comes back status 2 with the fixture's reason and block, and the call returns normally (the same inputs pass the
    one-lane host build of the decoder under AddressSanitizer first: tests/test_host_bgzf.py);
  - records, counts, .bin and .lib_info are those of the text route."""
import gzip
import os
import subprocess
import time

import numpy as np
import pytest

import bgzf_util as bz
import fastx_cases as fc
import golden_util as gu

pytestmark = pytest.mark.gpu


# ---- Engine.bgzf_inflate -------------------------------------------------------------------------------------------------------------

def test_well_formed_fixtures_inflate_to_zlibs_text(engine):
    for fx in bz.good_fixtures():
        r, text = engine.bgzf_inflate(fx.data)
        assert (r.status, r.reason) == (0, 0), "%s: status %d reason %d block %d" % (fx.name, r.status, r.reason, r.bad_block)
        assert (r.n_blocks, r.n_text) == (fx.n_blocks, len(fx.text)), fx.name
        assert text == fx.text, fx.name


def test_malformed_fixtures_are_declined_with_their_reason(engine):
    for fx in bz.bad_fixtures():
        r, text = engine.bgzf_inflate(fx.data)
        assert (r.status, r.reason, r.bad_block) == (2, fx.reason, fx.block), "%s: status %d reason %d block %d" % (fx.name, r.status, r.reason, r.bad_block)
        assert text is None
    # and the context is as good as before
    fx = bz.good_fixtures()[2]
    r, text = engine.bgzf_inflate(fx.data)
    assert r.status == 0 and text == fx.text


def test_an_empty_file_is_an_empty_text(engine):
    r, text = engine.bgzf_inflate(b"")
    assert (r.status, r.n_blocks, r.n_text, text) == (0, 0, 0, b"")


# ---- Engine.fastx_bgzf_to_records ----------------------------------------------------------------------------------------------------

def same_records(engine, name, t1, t2=None, block_size=1000):
    want, want_rec = engine.fastx_to_records(t1, t2)
    got, rec = engine.fastx_bgzf_to_records(bz.bgzf(t1, block_size), None if t2 is None else bz.bgzf(t2, block_size))
    assert got.status == want.status, "%s: status %d, the text route's %d" % (name, got.status, want.status)
    if want.status == 0:
        assert (got.n_reads, got.n_bases, got.n_words, got.max_len) == (want.n_reads, want.n_bases, want.n_words, want.max_len), name
        assert np.array_equal(rec, want_rec), name
    return got.status


def test_fixed_fasta_and_fastq_cases_as_bgzf_of_1000_byte_blocks(engine):
    """1000-byte blocks put block edges inside lines and headers"""
    for name, text in fc.fixed_fasta() + fc.fixed_fastq():
        same_records(engine, name, text)
    assert same_records(engine, "fq_lengths", dict(fc.fixed_fastq())["fq_lengths"]) == 0


def test_paired_files(engine):
    by_name = {n: (a, b) for n, a, b in fc.fixed_pairs()}
    for name in ("pe_fq_fq", "pe_fa_fq", "pe_300_records", "pe_one_empty", "pe_unequal_first_longer"):
        st = same_records(engine, name, *by_name[name])
        assert st == 0 or name in ("pe_one_empty", "pe_unequal_first_longer"), name


def test_a_crlf_text_is_status_1(engine):
    assert same_records(engine, "fq_crlf", dict(fc.declined_fastq())["fq_crlf"]) == 1


def test_a_file_that_is_not_bgzf_is_status_2(engine):
    text = dict(fc.fixed_fastq())["fq_lengths"]
    good = bz.bgzf(text, 1000)
    for gz1, gz2 in ((gzip.compress(text), None), (good, gzip.compress(text)), (bz.bad_fixtures()[7].data, None)):
        r, rec = engine.fastx_bgzf_to_records(gz1, gz2)
        assert r.status == 2 and rec is None


# ---- mhx_core buildlib ---------------------------------------------------------------------------------------------------------------

ROUTE = "blocks inflated on the GPU"


def buildlib(d, lib, out, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MHX_BUILDLIB")}
    e.update(env)
    p = subprocess.run([gu.MHX_CORE, "buildlib", lib, os.path.join(d, out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=e, timeout=120)
    files = None
    if p.returncode == 0:
        files = (open(os.path.join(d, out + ".bin"), "rb").read(), open(os.path.join(d, out + ".lib_info"), "rb").read())
    return p, files


@pytest.fixture(scope="module")
def lib_dir(tmp_path_factory):
    """se, pe and interleaved libraries as BGZF; a pe library with one plain-gzip mate and a plain-gzip se library; a corrupt BGZF file"""
    d = str(tmp_path_factory.mktemp("bgzf_lib"))
    pairs = {n: (a, b) for n, a, b in fc.fixed_pairs()}
    se = bz.fastq_text(700, 60, 21)
    inter = bz.fastq_text(400, 75, 22)
    m1, m2 = pairs["pe_300_records"]
    for name, data in (("se.fq.gz", bz.bgzf(se, 5000)), ("il.fq.gz", bz.bgzf(inter, 65280)), ("m1.fa.gz", bz.bgzf(m1, 1000)), ("m2.fq.gz", bz.bgzf(m2, 1000)),
                       ("m2_plain.fq.gz", gzip.compress(m2)), ("se_plain.fq.gz", gzip.compress(se)),
                       ("corrupt.fq.gz", bz.block(se[:5000]) + bz.block(se[5000:9000], crc=1) + bz.EOF_BLOCK)):
        open(os.path.join(d, name), "wb").write(data)
    p = lambda n: os.path.join(d, n)
    open(p("bgzf.lib"), "w").write("single\nse %s\nmates\npe %s %s\ninterleaved\ninterleaved %s\n" % (p("se.fq.gz"), p("m1.fa.gz"), p("m2.fq.gz"), p("il.fq.gz")))
    open(p("mixed.lib"), "w").write("mates\npe %s %s\nsingle\nse %s\n" % (p("m1.fa.gz"), p("m2_plain.fq.gz"), p("se_plain.fq.gz")))
    open(p("corrupt.lib"), "w").write("single\nse %s\n" % p("corrupt.fq.gz"))
    return d


def test_buildlib_writes_the_same_files_by_the_bgzf_route(lib_dir):
    d = lib_dir
    lib = os.path.join(d, "bgzf.lib")
    today, want = buildlib(d, lib, "today")
    assert today.returncode == 0 and ROUTE not in today.stderr, today.stderr[-600:]
    new, got = buildlib(d, lib, "new", MHX_BUILDLIB_BGZF="1")
    assert new.returncode == 0 and new.stderr.count(ROUTE) == 3, new.stderr[-600:]  # one line per library
    assert got == want
    host, got_host = buildlib(d, lib, "host", MHX_BUILDLIB_BGZF="1", MHX_BUILDLIB_HOST="1")  # the host parser wins over the new variable
    assert host.returncode == 0 and ROUTE not in host.stderr and got_host == want


def test_a_library_that_is_not_bgzf_throughout_takes_todays_route(lib_dir):
    d = lib_dir
    lib = os.path.join(d, "mixed.lib")
    host, want = buildlib(d, lib, "mixed_host", MHX_BUILDLIB_HOST="1")
    new, got = buildlib(d, lib, "mixed_new", MHX_BUILDLIB_BGZF="1")
    assert host.returncode == 0 and new.returncode == 0 and ROUTE not in new.stderr and got == want


def test_a_corrupt_bgzf_file_ends_as_it_ends_today(lib_dir):
    d = lib_dir
    lib = os.path.join(d, "corrupt.lib")
    today, _ = buildlib(d, lib, "corrupt_today")
    new, _ = buildlib(d, lib, "corrupt_new", MHX_BUILDLIB_BGZF="1")
    assert today.returncode != 0 and new.returncode == today.returncode and ROUTE not in new.stderr
    last = lambda p: [l for l in p.stderr.splitlines() if l.strip()][-1]
    assert "read error" in last(today) and last(new) == last(today)


def test_the_route_through_the_resident_server(lib_dir):
    d = lib_dir
    with gu.socket_dir() as sd:
        sock = os.path.join(sd, "mhx.sock")
        log = open(os.path.join(d, "server.log"), "w")
        srv = subprocess.Popen([gu.MHX_CORE, "--serve", sock], stdout=subprocess.DEVNULL, stderr=log, env=dict(os.environ, MHX_SERVE_IDLE_S="60"))
        try:
            for _ in range(500):
                if os.path.exists(sock):
                    break
                time.sleep(0.02)
            assert os.path.exists(sock)
            _, want = buildlib(d, os.path.join(d, "bgzf.lib"), "srv_host", MHX_BUILDLIB_HOST="1")
            p, got = buildlib(d, os.path.join(d, "bgzf.lib"), "srv_new", MHX_BUILDLIB_BGZF="1", MHX_SERVER=sock)
            assert p.returncode == 0 and p.stderr.count(ROUTE) == 3 and got == want, p.stderr[-600:]
            assert srv.poll() is None
        finally:
            subprocess.run([gu.MHX_CORE, "--serve-stop", sock], timeout=60)
            try:
                srv.wait(timeout=30)
            except subprocess.TimeoutExpired:
                srv.kill()
            log.close()
