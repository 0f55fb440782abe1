"""GPU: `mhx_core assemble` on its GPU routes (MHX_ASSEMBLE_BUBBLE=1: weak links, tips, low-depth pruning at levels 1 to 3, naive and
complex bubbles, Refresh, the finish) on the structured small graphs of tools/fuzz_assemble.py — tandem repeats shorter than k,
inverted repeats, hairpins, rings of a few edges, self-complementary rings, second haplotypes with indels, multiplicities past
the 8-bit field — with option sets drawn from the whole envelope `assemble_on_gpu()` serves.

(i) every committed seed against COMMITTED digests and counts of the reference's `assemble -t 1` (tests/golden/assemble_fuzz.json):
the library from the generator, the graph from `mhx_core read2sdbg`, every output file byte for byte, which files exist, the
logged counts.  Nothing of the reference is needed; MHX_REF_CORE points to a stub that fails, so forwarding cannot pass.
(ii) thirty seconds of the tool itself, live against the reference (skipped where the reference is not built), from a seed
outside the committed list."""
import json
import os
import subprocess
import sys

import pytest

import golden_util as gu

sys.path.insert(0, os.path.join(gu.ROOT, "tools"))
import fuzz_assemble as fa  # noqa: E402

pytestmark = pytest.mark.gpu

with open(fa.GOLDEN) as f:
    GOLDEN = json.load(f)["cases"]
LIVE_SEED0 = 500000  # the committed seeds are all below it


@pytest.mark.parametrize("g", GOLDEN, ids=lambda g: g["name"])
def test_a_committed_seed_matches_the_reference(g, tmp_path):
    c = fa.case(g["seed"])
    assert (c["k"], c["args"]) == (g["k"], g["args"])
    dig, log = fa.gpu_case(c, str(tmp_path))
    print(g["name"], fa.describe(c), fa.brief(log))
    assert log == g["log"]
    assert dig == g["digests"]  # (the files there are, and every one byte for byte)


@pytest.mark.skipif(not os.path.exists(fa.REF), reason="oracle/_ref/ref_megahit_core not built (no reference sources here)")
def test_thirty_seconds_of_structured_graphs():
    assert all(g["seed"] < LIVE_SEED0 for g in GOLDEN)
    p = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "fuzz_assemble.py"), "30", str(LIVE_SEED0)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "all equal to the reference" in p.stdout, p.stdout[-1500:]
