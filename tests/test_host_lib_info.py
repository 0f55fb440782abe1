"""CPU: the per-library lines of a read library's .lib_info through the CLI's host side (mhxio::read_lib_info_libs in
megahit_amd/csrc/host/formats.cpp), driven by tests/host/lib_info_check.cpp built here with g++."""
import os
import subprocess

import pytest

import local_cases
import local_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "megahit_amd", "csrc", "host")

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("lib_info")), "lib_info_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST, os.path.join(ROOT, "tests", "host", "lib_info_check.cpp"),
                    os.path.join(HOST, "formats.cpp"), "-lz", "-lpthread", "-o", path], check=True)
    return path


def test_libraries_of_a_collection(exe, tmp_path):
    i = next(j for j in U.SMALL if U.CASES[j]["name"] == "two_libs")
    _, prefix = local_cases.write_files(U.CASES[i], str(tmp_path))
    p = subprocess.run([exe, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr
    got = [l.split("|") for l in p.stdout.splitlines()]
    assert [tuple(int(x) for x in g[0].split()) for g in got] == [(b, e, m, int(pd)) for b, e, m, pd in U.inputs(i)["table"]]
    assert len(got) == 2 and all(g[1] == "synthetic" for g in got)


def test_truncated_file_is_an_error(exe, tmp_path):
    prefix = os.path.join(str(tmp_path), "bad")
    with open(prefix + ".lib_info", "w") as f:
        f.write("100 2\nsome library\n0 2\n")
    assert subprocess.run([exe, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 1
    with open(prefix + ".lib_info", "w") as f:
        f.write("100 2\nlib\n0 4 50 1\n")  # more reads than the totals say
    assert subprocess.run([exe, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 1
