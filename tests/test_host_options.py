"""CPU: the table of tuning knobs (megahit_amd/csrc/mhx_options.h: names, environment names, defaults, derived knobs), the rule that
resolves a knob (explicit option, environment, tuning file, default) and the scoped setter, driven by a small C++ program built here
with g++ (no GPU, no libmhx, no HIP header: the table is plain C++): tests/host/options_check.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "options_check.cpp")
GXX = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_the_table_the_precedence_and_the_scope(tmp_path):
    exe = os.path.join(str(tmp_path), "options_check")
    subprocess.run(GXX + ["-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MHX_")}
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr


@pytest.mark.parametrize("form", ["WRONG_FORM_PLAIN", "WRONG_FORM_DERIVED"])
def test_the_wrong_form_for_a_knob_does_not_compile(form):
    assert subprocess.run(GXX + ["-fsyntax-only"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 0
    p = subprocess.run(GXX + ["-fsyntax-only", "-D" + form], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode != 0 and "static assertion failed" in p.stderr and "opt<Opt::name>" in p.stderr, p.stderr
