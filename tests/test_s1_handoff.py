"""CPU: the record that holds what stage 1 leaves in the handle for stage 2 (megahit_amd/csrc/s1_handoff.h: aggregated items, their
digit histograms, stage 1's claim on the is_solid bitmap, the bound of the '$' items), driven through the library's sequences by a
small C++ program built here with g++ (no GPU, no libmhx, no HIP header: the record is plain C++): tests/host/s1_handoff_check.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_the_queries_after_every_step(tmp_path):
    exe = os.path.join(str(tmp_path), "s1_handoff_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "s1_handoff_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr

