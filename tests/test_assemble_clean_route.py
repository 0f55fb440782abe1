"""CPU: the opt-in route of `mhx_core assemble` with cleaning rounds.  With MHX_ASSEMBLE_CLEAN=1, --bubble_level 0
--prune_level 0 --cleaning_rounds N (N >= 1, the default 5 included) runs on the GPU; any other bubble or prune level and
MHX_ASSEMBLE_REF=1 still execv $MHX_REF_CORE with the command line unchanged; without the variable nothing changes —
checked with a stub that records its argv (nothing here starts a GPU)."""
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


def run(args, ref, clean, **extra):
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off", MHX_NO_FORK="1", **extra)
    for name in ("MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN"):
        if name not in extra:
            env.pop(name, None)
    if clean is not None:
        env["MHX_ASSEMBLE_CLEAN"] = clean
    return subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)


def qualifying(tmp_path):
    s, o = str(tmp_path / "missing"), str(tmp_path / "out")
    return [
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "0"],  # the default 5 rounds
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "1", "-t", "4"],
    ]


@pytest.mark.parametrize("which", [0, 1])
def test_cleaning_rounds_do_not_forward_when_opted_in(recorder, tmp_path, which):
    """the GPU route is taken (and, with no graph on disk, fails in the reader before any device work)"""
    ref, log = recorder
    p = run(qualifying(tmp_path)[which], ref, "1")
    assert p.returncode != 0
    assert "missing.sdbg_info" in p.stderr
    assert not log.exists()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("clean", [None, "0"])
def test_cleaning_rounds_forward_without_the_variable(recorder, tmp_path, which, clean):
    ref, log = recorder
    args = qualifying(tmp_path)[which]
    p = run(args, ref, clean)
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


STILL_FORWARDED = [
    ["-s", "g", "-o", "out"],  # the defaults: bubble level 2, prune level 2
    ["-s", "g", "-o", "out", "--bubble_level", "1", "--prune_level", "0", "--cleaning_rounds", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--cleaning_rounds", "1"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "1", "--cleaning_rounds", "3"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "3"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "-1"],
    ["-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "2"],  # no graph: the reference reports it
]


@pytest.mark.parametrize("args", STILL_FORWARDED, ids=range(len(STILL_FORWARDED)))
def test_other_levels_forward_when_opted_in(recorder, args):
    ref, log = recorder
    p = run(args, ref, "1")
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_assemble_ref_wins_over_the_opt_in(recorder, tmp_path):
    ref, log = recorder
    args = qualifying(tmp_path)[1]
    p = run(args, ref, "1", MHX_ASSEMBLE_REF="1")
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_no_cleaning_rounds_route_is_unchanged(recorder, tmp_path):
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out"), "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "0"]
    for clean in (None, "1"):
        p = run(args, ref, clean)
        assert p.returncode != 0
        assert "missing.sdbg_info" in p.stderr
        assert not log.exists()
