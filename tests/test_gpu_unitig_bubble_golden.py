"""GPU: `mhx_core assemble --bubble_level 1|2 --prune_level 0|2|3 [--careful_bubble]` with MHX_ASSEMBLE_BUBBLE=1 against COMMITTED
digests and counts of the reference's own `assemble -t 1` (tests/golden/unitig_bubble.json, tools/make_unitig_bubble_golden.py):
the graph from `mhx_core read2sdbg` on the same deterministic library (one graph per library, shared by its cases), every
output file byte for byte — .bubble_seq.fa with its records in the reference's order among them — and the logged counts: per
round "bubbles removed", "complex bubbles removed", "disconnected", "Tips removed", "removed in (more-)excessive pruning", the
final "local low depth / complex bubbles" pair, graph size and final statistics.  Nothing of the reference is needed at run
time; MHX_REF_CORE points to a stub that fails, so forwarding cannot pass."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_bubble_golden as mbg  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(gu.GOLD, "unitig_bubble.json")) as f:
    GOLDEN = json.load(f)["cases"]
SIMILARITY = r"Complex bubble candidates: (\d+), similarity passed: (\d+), failed: (\d+)"


@pytest.fixture(scope="module")
def graph_of(tmp_path_factory):
    """case -> prefix of its graph (mhx_core read2sdbg), built once per library"""
    made = {}

    def get(c):
        key = tuple(c.get(k) for k in mbg.LIBRARY)
        if key not in made:
            d = str(tmp_path_factory.mktemp("g"))
            g = os.path.join(d, "g")
            subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                            "--read_lib_file", mbg.write_library(d, c), "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []),
                           check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            made[key] = g
        return made[key]

    return get


@pytest.mark.parametrize("c", GOLDEN, ids=lambda c: c["name"])
def test_bubbles_match_the_committed_answer(c, graph_of, tmp_path):
    d = str(tmp_path)
    g = graph_of(c)
    stub = os.path.join(d, "ref_stub.sh")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(stub, 0o755)
    env = dict(os.environ, MHX_REF_CORE=stub, MHX_ASSEMBLE_BUBBLE="1")
    for name in ("MHX_SERVER", "MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE"):
        env.pop(name, None)
    out = os.path.join(d, "mine")
    p = subprocess.run([gu.MHX_CORE, "assemble", "-s", g, "-o", out] + mbg.assemble_args(c), env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = mbg.parse_log(p.stderr)
    got["bubble_records"] = mbg.records(out + ".bubble_seq.fa")
    got["addi_records"] = mbg.records(out + ".addi.fa") if c["prune"] >= 1 else 0
    print(c["name"], got, re.findall(SIMILARITY, p.stderr))
    assert got == c["log"]
    assert os.path.exists(out + ".addi.fa") == (c["prune"] >= 1)
    for s, want in c["digests"].items():
        with open(out + s, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want, s
    # some similarity check passes and some fails: at 0.95 bubbles pop; at 0.98 the same graph pops none of them although
    # they are candidates there too (see the case list of the generator)
    sims = [tuple(int(x) for x in t) for t in re.findall(SIMILARITY, p.stderr)]
    if c["name"] == "A-b2":
        assert sum(t[1] for t in sims) > 0
    if c["name"] == "A-b2-p0-sim0.98":
        assert sum(t[2] for t in sims) > 0 and sum(t[0] for t in sims) > 0
    if c["name"] in ("A-b2-merge0", "A-b2-early-return"):
        assert all(t == (0, 0, 0) for t in sims)  # the pass returned before it looked at the graph
