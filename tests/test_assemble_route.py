"""CPU: which `mhx_core assemble` command lines leave for the reference.  Only --bubble_level 0 --prune_level 0
--cleaning_rounds 0 runs on the GPU; every other option set, and MHX_ASSEMBLE_REF=1, still execv's $MHX_REF_CORE with
the command line unchanged — checked with a stub that records its argv (nothing here starts a GPU)."""
import os
import subprocess

import pytest

import golden_util as gu


@pytest.fixture
def recorder(tmp_path):
    log = tmp_path / "argv.txt"
    p = tmp_path / "ref_stub.sh"
    p.write_text('#!/bin/sh\nfor a in "$@"; do echo "$a"; done > "%s"\nexit 0\n' % log)
    p.chmod(0o755)
    return str(p), log


FORWARDED = [
    ["-s", "g", "-o", "out"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "1", "--cleaning_rounds", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--cleaning_rounds", "0", "--max_tip_len", "10"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "1", "-t", "4"],
    ["-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"],  # no graph: the reference reports it
    ["-s", "g", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0", "--no_such_option", "1"],
]


@pytest.mark.parametrize("args", FORWARDED, ids=range(len(FORWARDED)))
def test_other_option_sets_forward(recorder, args):
    ref, log = recorder
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off")
    env.pop("MHX_ASSEMBLE_REF", None)
    p = subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_assemble_ref_forces_forwarding(recorder):
    ref, log = recorder
    args = ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0", "--output_standalone"]
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_ASSEMBLE_REF="1", MHX_SERVER="off")
    p = subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_qualifying_options_do_not_forward(recorder, tmp_path):
    """the GPU route is taken (and, with no graph on disk, fails in the reader before any device work)"""
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out"), "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"]
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off", MHX_NO_FORK="1")
    env.pop("MHX_ASSEMBLE_REF", None)
    p = subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode != 0
    assert "missing.sdbg_info" in p.stderr
    assert not log.exists()
