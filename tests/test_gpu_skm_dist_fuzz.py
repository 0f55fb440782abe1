"""GPU: twenty seconds of tools/fuzz_skm_dist.py — random libraries on 2-9 thread ranks (sometimes one empty or degenerate shard)
through mhx_dist_read2sdbg with the super-k-mer exchange where the ranks take it, every output against the oracle on the union."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twenty_seconds_of_random_worlds():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_skm_dist.py"), "20", "91000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "all equal to the oracle" in p.stdout, p.stdout[-1500:]
