"""GPU: `mhx_core` count, seq2sdbg --need_mercy, read2sdbg and read2sdbg --need_mercy reproduce the REFERENCE's digests at
k = 45 .. 255 (tests/golden/wide_k.json, tools/make_wide_k_golden.py) on the seeded library of wide_k_cases; at k = 127 and 255
(tip labels of 8 and 16 words) the written SdBG files go through the device-resident index and the tip trimming, against the
reference's own loader where oracle/_ref/ref_sdbg_dump is built."""
import json
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import wide_k_cases as wk
from megahit_amd import lib
from test_gpu_sdbg_index import REF_DUMP, check_index, load_files_into, read_dump

pytestmark = pytest.mark.gpu

with open(os.path.join(gu.GOLD, "wide_k.json")) as _f:
    GOLDEN = json.load(_f)

_RUNS = {}


def run(k, tmp_path_factory):
    """the four mhx_core runs at k, once per session: (digests, prefixes of the SdBG files)"""
    if k not in _RUNS:
        d = str(tmp_path_factory.mktemp("wide_k%d" % k))
        _RUNS[k] = wk.run_four(gu.MHX_CORE, wk.write_library(d, GOLDEN["seed"], k), k, d)
    return _RUNS[k]


@pytest.mark.parametrize("ent", GOLDEN["cases"], ids=lambda c: "k%d" % c["k"])
def test_cli_reproduces_reference_at_wide_k(ent, tmp_path_factory):
    got, _ = run(ent["k"], tmp_path_factory)
    for key, want in ent.items():
        assert got[key] == want, key


@pytest.mark.skipif(not os.path.exists(REF_DUMP), reason="oracle/_ref/ref_sdbg_dump not built")
@pytest.mark.parametrize("which", ["read2sdbg_mercy", "seq2sdbg_mercy"])
@pytest.mark.parametrize("k", [127, 255])
def test_index_and_tip_trimming_equal_reference_loader(engine, k, which, tmp_path_factory, tmp_path):
    prefix = run(k, tmp_path_factory)[1][which]
    dump = os.path.join(str(tmp_path), "ref.dump")
    subprocess.run([REF_DUMP, prefix, dump, str(2 * k)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    want = read_dump(dump)
    assert int(want["meta"][0]) > 0 and int(want["meta"][1]) > 0 and int(want["meta"][4]) == (k + 15) // 16  # items, tips, label words
    assert load_files_into(engine, prefix) == k
    info = check_index(engine, k, want)
    assert np.array_equal(engine.fetch(lib.BUF_SDBG_INVALID, np.uint64), want["invalid"])
    assert engine.sdbg_remove_tips(info, 2 * k) == int(want["tips_removed"][0])
    assert np.array_equal(engine.fetch(lib.BUF_SDBG_INVALID, np.uint64), want["invalid_after_tips"])
