"""CPU: the opt-in route of `mhx_core assemble` with bubble popping.  With MHX_ASSEMBLE_BUBBLE=1, --bubble_level 0..2 with
--prune_level 0..3 (levels 1 to 3 with an explicit --min_depth > 0), --cleaning_rounds >= 0, with or without --careful_bubble
and --is_final_round, and --merge_len / --merge_similar inside the similarity kernel's cap runs on the GPU; the variable unset
or 0 — also next to MHX_ASSEMBLE_PRUNE=1 —, no --min_depth at a prune level >= 1, bubble level 3, a --merge_len beyond the cap
and MHX_ASSEMBLE_REF=1 still execv $MHX_REF_CORE with the command line unchanged.  Checked with a stub that records its argv
(nothing here starts a GPU)."""
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


def run(args, ref, bubble, **extra):
    env = dict(os.environ, MHX_REF_CORE=ref, MHX_SERVER="off", MHX_NO_FORK="1")
    for name in ("MHX_ASSEMBLE_REF", "MHX_ASSEMBLE_CLEAN", "MHX_ASSEMBLE_PRUNE", "MHX_ASSEMBLE_BUBBLE"):
        env.pop(name, None)
    env.update(extra)
    if bubble is not None:
        env["MHX_ASSEMBLE_BUBBLE"] = bubble
    return subprocess.run([gu.MHX_CORE, "assemble"] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=60)


def orchestrator(s, o, *more):
    """what the orchestrator passes by default (bubble level 2, prune level 2, merge 20 / 0.95) with a given depth"""
    return ["-s", s, "-o", o, "-t", "8", "--max_tip_len", "-1", "--min_standalone", "200", "--prune_level", "2", "--merge_len", "20",
            "--merge_similar", "0.95", "--cleaning_rounds", "5", "--disconnect_ratio", "0.1", "--low_local_ratio", "0.2", "--min_depth", "2",
            "--bubble_level", "2"] + list(more)


def qualifying(tmp_path):
    s, o = str(tmp_path / "missing"), str(tmp_path / "out")
    return [
        orchestrator(s, o),
        orchestrator(s, o, "--careful_bubble"),
        orchestrator(s, o, "--is_final_round"),
        orchestrator(s, o, "--careful_bubble", "--is_final_round"),
        ["-s", s, "-o", o, "--min_depth", "2"],  # assemble's own defaults: bubble level 2, prune level 2, 20 / 0.98
        ["-s", s, "-o", o, "--bubble_level", "1", "--prune_level", "0"],  # no depth needed at prune level 0
        ["-s", s, "-o", o, "--bubble_level", "1", "--prune_level", "3", "--min_depth", "1.5", "--careful_bubble"],
        ["-s", s, "-o", o, "--bubble_level", "2", "--prune_level", "3", "--min_depth", "2", "--cleaning_rounds", "0"],
        ["-s", s, "-o", o, "--bubble_level", "2", "--prune_level", "1", "--min_depth", "2", "--merge_len", "0"],
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "3", "--min_depth", "2"],  # prune level 3 without bubbles
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "2", "--min_depth", "2"],  # implies the pruning route
        ["-s", s, "-o", o, "--bubble_level", "0", "--prune_level", "0", "--cleaning_rounds", "2"],  # ... and the cleaning rounds
        ["-s", s, "-o", o, "--bubble_level", "2", "--prune_level", "0", "--merge_len", "60", "--merge_similar", "0.95"],  # the cap itself
    ]


N = 13


@pytest.mark.parametrize("which", range(N))
def test_bubbles_do_not_forward_when_opted_in(recorder, tmp_path, which):
    """the GPU route is taken (and, with no graph on disk, fails in the reader before any device work)"""
    ref, log = recorder
    args = qualifying(tmp_path)
    assert len(args) == N
    p = run(args[which], ref, "1")
    assert p.returncode != 0
    assert "missing.sdbg_info" in p.stderr
    assert not log.exists()


@pytest.mark.parametrize("which", range(10))  # (cases 10 and 11 are the pruning route's and the cleaning route's own)
@pytest.mark.parametrize("bubble,prune", [(None, None), ("0", None), (None, "1"), ("0", "1")])
def test_bubbles_forward_without_the_variable(recorder, tmp_path, which, bubble, prune):
    """unset or 0, also with MHX_ASSEMBLE_PRUNE=1, which alone still forwards bubble levels 1-2 and prune level 3"""
    ref, log = recorder
    args = qualifying(tmp_path)[which]
    p = run(args, ref, bubble, **({"MHX_ASSEMBLE_PRUNE": prune} if prune else {}))
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


STILL_FORWARDED = [
    ["-s", "g", "-o", "out"],  # prune level 2 without --min_depth: InferMinDepth is the reference's
    ["-s", "g", "-o", "out", "--bubble_level", "1", "--prune_level", "1"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "3", "--min_depth", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "2", "--min_depth", "-1"],
    ["-s", "g", "-o", "out", "--bubble_level", "3", "--prune_level", "2", "--min_depth", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "3", "--prune_level", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "4", "--min_depth", "2"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "2", "--min_depth", "2", "--cleaning_rounds", "-1"],
    # beyond the cap at k = 255: lround(61 * 255 / 0.95) + 255 = 16629 > 16384 characters
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--merge_len", "61", "--merge_similar", "0.95"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "2", "--min_depth", "2", "--merge_len", "1000"],
    # max_indel = (int)((lround(20 * 255 / 0.5) + 255) * 0.5) = 5227 > 2047 band half-width
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--merge_len", "20", "--merge_similar", "0.5"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--merge_similar", "0"],
    ["-s", "g", "-o", "out", "--bubble_level", "2", "--prune_level", "0", "--merge_similar", "1.5"],
    ["-o", "out", "--bubble_level", "1", "--prune_level", "0"],  # no graph: the reference reports it
]


@pytest.mark.parametrize("args", STILL_FORWARDED, ids=range(len(STILL_FORWARDED)))
def test_other_option_sets_forward_when_opted_in(recorder, args):
    ref, log = recorder
    p = run(args, ref, "1")
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args


def test_a_merge_len_beyond_the_cap_is_fine_below_bubble_level_2(recorder, tmp_path):
    """the cap is the complex remover's: bubble level 1 never compares strings"""
    ref, log = recorder
    p = run(["-s", str(tmp_path / "missing"), "-o", "out", "--bubble_level", "1", "--prune_level", "0", "--merge_len", "1000"], ref, "1")
    assert p.returncode != 0 and "missing.sdbg_info" in p.stderr and not log.exists()


@pytest.mark.parametrize("which", [0, 1, 6])
def test_assemble_ref_wins_over_the_opt_in(recorder, tmp_path, which):
    ref, log = recorder
    args = qualifying(tmp_path)[which]
    p = run(args, ref, "1", MHX_ASSEMBLE_REF="1")
    assert p.returncode == 0, p.stderr
    assert log.read_text().split("\n")[:-1] == ["assemble"] + args
