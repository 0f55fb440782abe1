"""CPU: the second opt-in level of `mhx_core assemble`.  MHX_ASSEMBLE_PRUNE=2 / MHX_ASSEMBLE_BUBBLE=2 is the route of level 1 plus
the command lines at a prune level >= 1 that carry no --min_depth > 0: the depth is then inferred on the device
(mhx_sdbg_infer_min_depth).  At level 1 those command lines are forwarded as they always were (tests/test_assemble_prune_route.py,
tests/test_assemble_bubble_route.py hold that); every other rule is the same at both levels.  Checked with a stub that records
its argv (nothing here starts a GPU)."""
import os
import subprocess

import pytest

import golden_util as gu

PRUNE_NO_DEPTH = [  # the lines tests/test_assemble_prune_route.py STILL_FORWARDED[:4] forwards at level 1
    ["--bubble_level", "0"],
    ["--bubble_level", "0", "--prune_level", "1"],
    ["--bubble_level", "0", "--prune_level", "2", "--min_depth", "0"],
    ["--bubble_level", "0", "--prune_level", "2", "--min_depth", "-1"],
]
BUBBLE_NO_DEPTH = [  # tests/test_assemble_bubble_route.py STILL_FORWARDED[:4]
    [],  # the bare `assemble -s g -o out`
    ["--bubble_level", "1", "--prune_level", "1"],
    ["--bubble_level", "2", "--prune_level", "3", "--min_depth", "0"],
    ["--bubble_level", "2", "--prune_level", "2", "--min_depth", "-1"],
    # what the orchestrator passes for --prune-level 3 without --prune-depth
    ["--bubble_level", "2", "--prune_level", "3", "--careful_bubble", "--min_depth", "-1", "--merge_len", "20", "--merge_similar", "0.95"],
]
STILL_FORWARDED_AT_2 = [  # (variable, options): the depth is not what forwards these
    ("MHX_ASSEMBLE_PRUNE", ["--bubble_level", "1", "--prune_level", "2"]),
    ("MHX_ASSEMBLE_PRUNE", ["--bubble_level", "0", "--prune_level", "3"]),
    ("MHX_ASSEMBLE_PRUNE", ["--bubble_level", "0", "--prune_level", "2", "--cleaning_rounds", "-1"]),
    ("MHX_ASSEMBLE_BUBBLE", ["--bubble_level", "3", "--prune_level", "2"]),
    ("MHX_ASSEMBLE_BUBBLE", ["--bubble_level", "2", "--prune_level", "4"]),
    ("MHX_ASSEMBLE_BUBBLE", ["--bubble_level", "2", "--prune_level", "2", "--merge_len", "1000"]),
]


@pytest.fixture
def recorder(tmp_path):
    log = tmp_path / "argv.txt"
    p = tmp_path / "ref_stub.sh"
    p.write_text('#!/bin/sh\nfor a in "$@"; do echo "$a"; done > "%s"\nexit 0\n' % log)
    p.chmod(0o755)
    return str(p), log


def run(args, ref, **extra):
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off", MHX_NO_FORK="1")
    for name in ("MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE", "MHX_ASSEMBLE_BUBBLE"):
        env.pop(name, None)
    env.update(extra)
    return subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)


CASES = [("MHX_ASSEMBLE_PRUNE", o) for o in PRUNE_NO_DEPTH] + [("MHX_ASSEMBLE_BUBBLE", o) for o in PRUNE_NO_DEPTH + BUBBLE_NO_DEPTH]


@pytest.mark.parametrize("var,opts", CASES, ids=range(len(CASES)))
def test_no_depth_is_served_at_level_2_and_forwarded_at_level_1(recorder, tmp_path, var, opts):
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out")] + opts
    p = run(args, ref, **{var: "2"})  # the GPU route is taken (and, with no graph on disk, fails in the reader before any device work)
    assert p.returncode != 0 and "missing.sdbg_info" in p.stderr and not log.exists()
    p = run(args, ref, **{var: "1"})
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


@pytest.mark.parametrize("var,opts", STILL_FORWARDED_AT_2, ids=range(len(STILL_FORWARDED_AT_2)))
def test_other_rules_hold_at_level_2(recorder, tmp_path, var, opts):
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out")] + opts
    p = run(args, ref, **{var: "2"})
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_level_2_of_the_pruning_variable_does_not_open_the_bubble_route(recorder, tmp_path):
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out")]  # bubble level 2 by default
    assert run(args, ref, MHX_ASSEMBLE_PRUNE="2").returncode == 0 and log.exists()


def test_assemble_ref_wins_at_level_2(recorder, tmp_path):
    ref, log = recorder
    args = ["-s", str(tmp_path / "missing"), "-o", str(tmp_path / "out"), "--bubble_level", "0"]
    p = run(args, ref, MHX_ASSEMBLE_PRUNE="2", MHX_ASSEMBLE_REF="1")
    assert p.returncode == 0 and log.read_text().split("\n")[:-1] == ["assemble"] + args
