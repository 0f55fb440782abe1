"""CPU: the rounds and the plan of the giant bins in slices (megahit_amd/csrc/skm_giant.h: which keys a round takes, the round behind a
round of a traversal that starts at any (sub0, rj0), and the depth every giant bin gets from its records, the job's records and the
knobs), driven by a small C++ program built here with g++ and with ROCm's clang++ under the address and undefined-behaviour sanitizers
(no GPU, no libmhx, no HIP header: the header is plain C++): tests/host/skm_giant_check.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")

ROCM_CLANG = "/opt/rocm/llvm/bin/clang++"
COMPILERS = [pytest.param("g++", marks=pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")),
             pytest.param(ROCM_CLANG, marks=pytest.mark.skipif(not os.path.exists(ROCM_CLANG), reason="needs ROCm's clang++"), id="rocm-clang++")]


@pytest.mark.parametrize("cxx", COMPILERS)
def test_the_rounds_and_the_plan_against_their_definitions(tmp_path, cxx):
    exe = os.path.join(str(tmp_path), "skm_giant_check")
    subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "skm_giant_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr
