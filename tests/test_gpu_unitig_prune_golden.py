"""GPU: `mhx_core assemble --bubble_level 0 --prune_level 1|2 --min_depth D` with MHX_ASSEMBLE_PRUNE=1 against COMMITTED digests
and counts of the reference's own `assemble -t 1` (tests/golden/unitig_prune.json, tools/make_unitig_prune_golden.py): the
graph from `mhx_core read2sdbg` on the same deterministic library (one graph per library, shared by its cases), all eight
output files byte for byte, and the logged counts: per round "disconnected", "Tips removed" and "removed in excessive
pruning", the "local low depth unitigs removed", graph size and final statistics.  Nothing of the reference is needed at run
time; MHX_REF_CORE points to a stub that fails, so forwarding cannot pass."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_prune_golden as mpg  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(gu.GOLD, "unitig_prune.json")) as f:
    GOLDEN = json.load(f)["cases"]
LIBRARY = ("kind", "G", "pairs", "err", "seed", "read_len", "frag", "k", "m", "mercy", "plasmid")


@pytest.fixture(scope="module")
def graph_of(tmp_path_factory):
    """case -> prefix of its graph (mhx_core read2sdbg), built once per library"""
    made = {}

    def get(c):
        key = tuple(c.get(k) for k in LIBRARY)
        if key not in made:
            d = str(tmp_path_factory.mktemp("g"))
            g = os.path.join(d, "g")
            subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                            "--read_lib_file", mpg.mcg.write_library(d, c), "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []),
                           check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            made[key] = g
        return made[key]

    return get


@pytest.mark.parametrize("c", GOLDEN, ids=lambda c: c["name"])
def test_pruning_matches_the_committed_answer(c, graph_of, tmp_path):
    d = str(tmp_path)
    g = graph_of(c)
    stub = os.path.join(d, "ref_stub.sh")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(stub, 0o755)
    env = dict(os.environ, MHX_REF_CORE=stub, MHX_ASSEMBLE_PRUNE="1")
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN"):
        env.pop(name, None)
    out = os.path.join(d, "mine")
    p = subprocess.run([gu.MHX_CORE, "assemble", "-s", g, "-o", out] + mpg.assemble_args(c), env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = mpg.parse_log(p.stderr)
    got["addi_records"] = mpg.addi_records(out)
    assert got == c["log"]
    for s in mpg.FILES:
        with open(out + s, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == c["digests"][s], s
