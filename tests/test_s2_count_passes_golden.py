"""CPU: tests/golden/s2_count_passes.json (tools/make_s2_count_passes_golden.py) has the shape tests/test_gpu_s2_count_passes_cli.py reads,
and holds digests only."""
import json
import os
import re

import golden_util as gu

MD5 = re.compile(r"^[0-9a-f]{32}$")


def test_golden_file_shape():
    path = os.path.join(gu.GOLD, "s2_count_passes.json")
    assert os.path.getsize(path) < 4096
    with open(path) as f:
        gold = json.load(f)
    assert set(gold) == {"library", "cases"}
    lib = gold["library"]
    assert MD5.match(lib["bin_md5"])
    assert (lib["reads"], lib["bases"], lib["read_len"]) == (200000, 20000000, 100)
    assert all(isinstance(v, (int, float)) for key, v in lib.items() if key != "bin_md5")
    assert sorted((e["k"], e["m"]) for e in gold["cases"]) == [(25, 2), (27, 1)]
    for e in gold["cases"]:
        assert set(e) == ({"k", "m", "sdbg"} if e["m"] == 1 else {"k", "m", "sdbg", "counting"})  # (min count 1 skips stage 1: no .counting)
        assert all(MD5.match(e[key]) for key in e if key not in ("k", "m"))
