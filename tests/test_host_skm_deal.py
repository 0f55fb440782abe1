"""CPU: the index arithmetic of the dealing in stage 1's group-by (megahit_amd/csrc/skm_deal.h: the record and the index within it of a
dealt window from the bitmap of run heads, the carry from chunk to chunk, a window's reverse complement from the window itself), driven
by a small C++ program built here with g++ and with ROCm's clang++ under the address and undefined-behaviour sanitizers (no GPU, no libmhx, no HIP header: the
header is plain C++): tests/host/skm_deal_check.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")

ROCM_CLANG = "/opt/rocm/llvm/bin/clang++"
# g++ takes the header's portable bit reversal, clang++ (the compiler of the kernels) the builtin the GPU code is made from: both are checked
COMPILERS = [pytest.param("g++", marks=pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")),
             pytest.param(ROCM_CLANG, marks=pytest.mark.skipif(not os.path.exists(ROCM_CLANG), reason="needs ROCm's clang++"), id="rocm-clang++")]


@pytest.mark.parametrize("cxx", COMPILERS)
def test_the_arithmetic_against_the_plain_definitions(tmp_path, cxx):
    exe = os.path.join(str(tmp_path), "skm_deal_check")
    subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "skm_deal_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr
