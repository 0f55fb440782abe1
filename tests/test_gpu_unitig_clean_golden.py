"""GPU: `mhx_core assemble --bubble_level 0 --prune_level 0 --cleaning_rounds N` with MHX_ASSEMBLE_CLEAN=1 against COMMITTED
digests and counts of the reference's own `assemble -t 1` (tests/golden/unitig_clean.json,
tools/make_unitig_clean_golden.py): the graph from `mhx_core read2sdbg` on the same deterministic library, all six output files
byte for byte, and the logged per-round "disconnected" / "Tips removed" counts, graph size and final statistics.  Nothing of
the reference is needed at run time; MHX_REF_CORE points to a stub that fails, so forwarding cannot pass."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import make_unitig_clean_golden as mcg  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(gu.GOLD, "unitig_clean.json")) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.mark.parametrize("c", GOLDEN, ids=lambda c: c["name"])
def test_cleaning_matches_the_committed_answer(c, tmp_path):
    d = str(tmp_path)
    lib = mcg.write_library(d, c)
    g = os.path.join(d, "g")
    subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--host_mem", "2e9", "--num_cpu_threads", "4",
                    "--read_lib_file", lib, "--output_prefix", g] + (["--need_mercy"] if c["mercy"] else []), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    stub = os.path.join(d, "ref_stub.sh")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\necho 'mhx_core forwarded to MHX_REF_CORE' >&2\nexit 97\n")
    os.chmod(stub, 0o755)
    env = dict(os.environ, MHX_REF_CORE=stub, MHX_ASSEMBLE_CLEAN="1")
    env.pop("MHX_SERVER", None)
    env.pop("MHX_ASSEMBLE_REF", None)
    out = os.path.join(d, "mine")
    p = subprocess.run([gu.MHX_CORE, "assemble", "-s", g, "-o", out] + mcg.assemble_args(c), env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert mcg.parse_log(p.stderr) == c["log"]
    for s in mcg.FILES:
        with open(out + s, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == c["digests"][s], s
