"""CPU: the opt-in route of `mhx_core assemble` with low-depth pruning.  With MHX_ASSEMBLE_PRUNE=1, --bubble_level 0
--prune_level 1|2 with an explicit --min_depth > 0 and --cleaning_rounds >= 0 runs on the GPU (and the variable implies the
cleaning rounds of MHX_ASSEMBLE_CLEAN); no or no positive --min_depth, bubble level 1 or 2, prune level 3, negative rounds,
MHX_ASSEMBLE_REF=1 and the variable unset or 0 — also next to MHX_ASSEMBLE_CLEAN=1 — still execv $MHX_REF_CORE with the
command line unchanged.  Checked with a stub that records its argv (nothing here starts a GPU)."""
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


def run(args, ref, prune, **extra):
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off", MHX_NO_FORK="1")
    for name in ("MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE"):
        env.pop(name, None)
    env.update(extra)
    if prune is not None:
        env["MHX_ASSEMBLE_PRUNE"] = prune
    return subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)


def qualifying(tmp_path):
    s, o = str(tmp_path / "missing"), str(tmp_path / "out")
    return [
        ["-s", s, "-o", o, "--bubble_level", "0", "--min_depth", "2"],  # the defaults: prune level 2, 5 rounds
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "2", "--min_depth", "2", "--is_final_round", "-t", "4"],
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "1", "--min_depth", "1.5", "--cleaning_rounds", "3"],
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "1", "--min_depth", "2", "--cleaning_rounds", "0", "--low_local_ratio", "0.05"],
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "2"],  # implies the cleaning rounds
        # what the orchestrator passes at --bubble-level 0
        ["-s", s, "-o", o, "-t", "8", "--max_tip_len", "-1", "--min_standalone", "200", "--prune_level", "2", "--merge_len", "20", "--merge_similar",
         "0.95", "--cleaning_rounds", "5", "--disconnect_ratio", "0.1", "--low_local_ratio", "0.2", "--min_depth", "2", "--bubble_level", "0"],
    ]


@pytest.mark.parametrize("which", range(6))
def test_pruning_does_not_forward_when_opted_in(recorder, tmp_path, which):
    """the GPU route is taken (and, with no graph on disk, fails in the reader before any device work)"""
    ref, log = recorder
    p = run(qualifying(tmp_path)[which], ref, "1")
    assert p.returncode != 0
    assert "missing.sdbg_info" in p.stderr
    assert not log.exists()


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("prune,clean", [(None, None), ("0", None), (None, "1"), ("0", "1")])
def test_pruning_forwards_without_the_variable(recorder, tmp_path, which, prune, clean):
    """unset or 0, also with MHX_ASSEMBLE_CLEAN=1 (which keeps its own prune-level-0 route: case 4)"""
    ref, log = recorder
    args = qualifying(tmp_path)[which]
    p = run(args, ref, prune, **({"MHX_ASSEMBLE_CLEAN": clean} if clean else {}))
    if which == 4 and clean == "1":
        assert p.returncode != 0 and "missing.sdbg_info" in p.stderr and not log.exists()
        return
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


STILL_FORWARDED = [
    ["-s", "g", "-o", "out", "--bubble_level", "0"],  # no --min_depth: InferMinDepth is the reference's
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "1"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "2", "--min_depth", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "2", "--min_depth", "-1"],
    ["-s", "g", "-o", "out", "--min_depth", "2"],  # the default bubble level 2
    ["-s", "g", "-o", "out", "--bubble_level", "1", "--prune_level", "2", "--min_depth", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "1", "--min_depth", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "1", "--prune_level", "0", "--cleaning_rounds", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "3", "--min_depth", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "2", "--min_depth", "2", "--cleaning_rounds", "-1"],
    ["-s", "g", "-o", "out", "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "-1"],
    ["-o", "out", "--bubble_level", "0", "--prune_level", "2", "--min_depth", "2"],  # no graph: the reference reports it
]


@pytest.mark.parametrize("args", STILL_FORWARDED, ids=range(len(STILL_FORWARDED)))
def test_other_option_sets_forward_when_opted_in(recorder, args):
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
