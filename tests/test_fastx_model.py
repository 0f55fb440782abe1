"""CPU: the reader model of tests/fastx_model.py is the reference's reader.  Every text of tests/fastx_cases.py goes into
`se`, `interleaved` and `pe` libraries; the reference's buildlib (oracle/_ref/ref_core) and the sequential parser of
`mhx_core buildlib` (MHX_BUILDLIB_HOST=1, no GPU involved) must both write exactly the .bin bytes and the .lib_info the
model predicts.  Only then may the model judge the GPU parser (tests/test_gpu_fastx_edges.py)."""
import os
import subprocess

import numpy as np
import pytest

import fastx_cases as fc
import fastx_model as fm
import golden_util as gu

needs_binaries = pytest.mark.skipif(not os.path.exists(gu.REF_CORE) or not os.path.exists(gu.MHX_CORE), reason="needs oracle/_ref/ref_core and mhx_core")


def test_generated_plain_texts_are_plain_and_declined_shapes_are_not():
    for name, text in fc.plain_singles():
        assert fm.plain(text), name
        assert all(b in (9, 10) or 0x20 <= b <= 0x7E for b in set(text)), name
    for name, text in fc.declined_fastq():
        assert not fm.plain(text), name
    for name, t1, t2 in fc.random_pairs():
        assert fm.plain(t1) and fm.plain(t2) and len(fm.records(t1)) == len(fm.records(t2)), name
    for name, text in fc.random_texts():
        assert len(text) <= 20000, name
    assert fm.plain(fc.carry_text_and_record()[0])
    assert not fm.plain(b">a\nACGT\n>") and not fm.plain(b">")


def test_model_on_the_texts_the_reference_was_probed_with():
    for text, n in ((b">a\nACGT\n>", 1), (b">", 0), (b">a\nACGT\n>\n", 2), (b">a\nACGT\n>b", 2)):
        assert len(fm.records(text)) == n, text
    assert fm.records(b">a x\nAC\n\nGT\n@q\nTT\n+\nII\nzz>b\nA>C") == [b"ACGT", b"TT", b"A>C"]
    assert fm.records(b">a\r\n\r\nAC\r\n\r\nG\r\n") == [b"\rACG"]  # a '\r' that is the whole accumulated string stays
    words, n_reads, n_bases, max_len = fm.pack([b"NNACGTNNACGT", b"nn", b"ACGTRYKMACGTACGTT"])
    assert (n_reads, n_bases, max_len) == (3, 4 + 1 + 17, 17)
    assert list(words) == [4, 0x1B000000, 1, 0, 17, 0x1B001B1B, 0xC0000000]


def _libraries():
    """-> {lib file name: [(meta, type, [texts], expected (words, n_reads, n_bases, max_len))]}"""
    singles = fc.all_singles()
    exp = {name: fm.expected(text) for name, text in singles}
    carry_text, carry_rec = fc.carry_text_and_record()
    se = [(name, "se", [text], exp[name]) for name, text in singles]
    se.append(("fa_carry", "se", [carry_text], (carry_rec, 1, fc.CARRY_LINES, fc.CARRY_LINES)))
    il = [(name, "interleaved", [text], exp[name]) for name, text in singles if exp[name][1] % 2 == 0]
    pe = [(name, "pe", [t1, t2], fm.expected(t1, t2)) for name, t1, t2 in fc.all_pairs()]
    assert len(il) > 20
    return {"se": se, "interleaved": il, "pe": pe}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """every library built once by the reference and once by the sequential parser -> {kind: (libs, {tag: (bin bytes, lib_info)})}"""
    d = str(tmp_path_factory.mktemp("fastx_model"))
    out = {}
    for kind, libs in _libraries().items():
        spec = []
        for i, (meta, ty, texts, _e) in enumerate(libs):
            paths = []
            for j, text in enumerate(texts):
                paths.append(os.path.join(d, "%s_%d_%d.txt" % (kind, i, j)))
                with open(paths[-1], "wb") as f:
                    f.write(text)
            spec.append("%s\n%s %s\n" % (meta, ty, " ".join(paths)))
        libf = os.path.join(d, kind + ".lib")
        with open(libf, "w") as f:
            f.write("".join(spec))
        got = {}
        for tag, exe, env in (("ref", gu.REF_CORE, {}), ("host", gu.MHX_CORE, {"MHX_BUILDLIB_HOST": "1"})):
            prefix = os.path.join(d, kind + "_" + tag)
            p = subprocess.run([exe, "buildlib", libf, prefix], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
            assert p.returncode == 0, p.stderr[-1500:]
            with open(prefix + ".bin", "rb") as f, open(prefix + ".lib_info") as g:
                got[tag] = (f.read(), g.read())
        out[kind] = (libs, got)
    return out


def check_against_model(libs, bin_bytes, lib_info):
    info = lib_info.split("\n")
    got = np.frombuffer(bin_bytes, dtype=np.uint32)
    reads = bases = pos = 0
    for i, (meta, ty, _texts, (words, n_reads, n_bases, max_len)) in enumerate(libs):
        assert info[1 + 2 * i] == meta
        assert info[2 + 2 * i] == "%d %d %d %d" % (reads, reads + n_reads, max_len, ty != "se"), meta
        assert np.array_equal(got[pos:pos + words.size], words), meta
        reads += n_reads
        bases += n_bases
        pos += words.size
    assert info[0] == "%d %d" % (bases, reads)
    assert info[1 + 2 * len(libs):] == [""] and pos == got.size and len(bin_bytes) % 4 == 0


@needs_binaries
@pytest.mark.parametrize("kind", ["se", "interleaved", "pe"])
def test_reference_buildlib_writes_what_the_model_says(built, kind):
    libs, got = built[kind]
    check_against_model(libs, *got["ref"])


@needs_binaries
@pytest.mark.parametrize("kind", ["se", "interleaved", "pe"])
def test_sequential_parser_writes_what_the_model_says(built, kind):
    libs, got = built[kind]
    check_against_model(libs, *got["host"])
