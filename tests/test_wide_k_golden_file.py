"""CPU: the C oracle (oracle_core) reproduces what the REFERENCE produced at wide k (tests/golden/wide_k.json, written by
tools/make_wide_k_golden.py from oracle/_ref/ref_core): count, seq2sdbg --need_mercy, read2sdbg and read2sdbg --need_mercy on
wide_k_cases.library at k = 45 .. 255, the widths at which the GPU tests rely on the oracle."""
import json
import os

import pytest

import golden_util as gu
import wide_k_cases as wk


def golden():
    with open(os.path.join(gu.GOLD, "wide_k.json")) as f:
        return json.load(f)


def test_golden_file_covers_the_k_list():
    g = golden()
    assert g["seed"] == wk.SEED and tuple(c["k"] for c in g["cases"]) == wk.K_GOLDEN
    for c in g["cases"]:  # no empty case
        assert c["n_edges"] > 0 and c["n_seq2sdbg_mercy"] > 0 and c["n_read2sdbg"] > 0 and c["n_read2sdbg_mercy"] > 0
    # mercy edges change the graph (a mercy edge may replace two dummy records: the record count alone can stay)
    assert all(c["read2sdbg_mercy"] != c["read2sdbg"] for c in g["cases"])


def test_k_sets_meet_every_width():
    assert {wk.s1_kw(k) for k in wk.K_ALL} == set(range(1, 18))
    assert {(k + 15) // 16 for k in wk.K_ALL} == set(range(1, 17))
    assert {wk.edge_words(k) for k in wk.K_EDGE_WORDS} == set(range(2, 18))
    for j in range(1, 16):  # both sides of every width boundary
        assert wk.s1_kw(16 * j - 3) + 1 == wk.s1_kw(16 * j - 1) and (16 * j + 15) // 16 + 1 == (16 * j + 1 + 15) // 16
        assert wk.edge_words(16 * j + 7) + 1 == wk.edge_words(16 * j + 9)


@pytest.mark.parametrize("ent", golden()["cases"], ids=lambda c: "k%d" % c["k"])
def test_oracle_reproduces_reference_at_wide_k(ent, tmp_path):
    gu.ensure_oracle()
    d = str(tmp_path)
    got, _ = wk.run_four(gu.ORACLE_CORE, wk.write_library(d, golden()["seed"], ent["k"]), ent["k"], d, ent["m"])
    assert got == ent
