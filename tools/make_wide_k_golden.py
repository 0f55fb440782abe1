"""Known answers of the reference at wide k, for tests that must not need the reference at run time (tests/golden/wide_k.json):
per k in wide_k_cases.K_GOLDEN the seeded library wide_k_cases.library(SEED, k) is written as a read library and
oracle/_ref/ref_core runs count, seq2sdbg --need_mercy on the count's edges, read2sdbg and read2sdbg --need_mercy (m = 2).
Only the digests (megahit_amd/canon.py) and the record counts are stored.
Run where oracle/_ref is built:   python tools/make_wide_k_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
import wide_k_cases as wk  # noqa: E402


def main():
    cases = []
    for k in wk.K_GOLDEN:
        with tempfile.TemporaryDirectory() as d:
            got, _ = wk.run_four(gu.REF_CORE, wk.write_library(d, wk.SEED, k), k, d)
        cases.append(got)
        print(k, got["n_edges"], got["n_seq2sdbg_mercy"], got["n_read2sdbg"], got["n_read2sdbg_mercy"], flush=True)
    with open(os.path.join(gu.GOLD, "wide_k.json"), "w") as f:
        json.dump({"seed": wk.SEED, "cases": cases}, f, indent=1)
    print("%d cases -> tests/golden/wide_k.json" % len(cases))


if __name__ == "__main__":
    main()
