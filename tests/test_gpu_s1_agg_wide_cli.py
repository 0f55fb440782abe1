"""GPU: `mhx_core read2sdbg -k 27 -m 2` with MHX_S1_AGG_WIDE=1 — stage 1 leaves stage 2's aggregated items (s1.hip S1Stage, s1_agg_wide) —
writes the files of the run without the knob, says so in its plan line, and every stage holds, over what was held when its plan was
made, at most the bytes it planned with (tests/test_gpu_memory_plan.py: peak - held <= budget): on the whole device, and on a device
faked so small that stage 1 runs in bucket-range passes whose items add up (no golden case of tests/golden is at k = 27: the
reference of the comparison is the knob-off run, which tests/test_gpu_memory_plan.py holds to the reference binary's route)."""
import os

import pytest

import golden_util as gu
from megahit_amd import canon, synth
from test_gpu_memory_plan import _check_budget, _core, _stages

pytestmark = pytest.mark.gpu

K, M = 27, 2
MARKER = "[aggregated stage-2 items, 6 count bits]"


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """(arguments, bases, digests of the knob-off run)"""
    d = str(tmp_path_factory.mktemp("aggwide"))
    reads = synth.gen_pe_reads(100000, 2000000, read_len=100, frag=250, err=0.005, seed=52)  # (the size the model below was made for)
    prefix = os.path.join(d, "lib")
    _, bases = synth.write_read_lib(prefix, [reads])
    args = ["read2sdbg", "-k", str(K), "-m", str(M), "--read_lib_file", prefix]
    out = os.path.join(d, "off")
    err = _core(gu.MHX_CORE, args, out, env={"MHX_S1_AGG_WIDE": "0"})
    assert "[aggregated stage-2 items" not in err
    return args, bases, {"sdbg": canon.digest_sdbg(out), "counting": canon.digest_file(out + ".counting")}


# small: MHX_FREE_BYTES = 30 per base.  By the model of tests/test_gpu_memory_plan.py stage 1 has avail = 0.7336 * 30 - fixed' per base with
# fixed' >= 1 + 1/8 + 1 (mark map, bitmap, the items kept for stage 2), and an item of a pass takes 17/16 * (24.5 + 0.25 + 8 + 16/63) =
# 35.1 bytes; the library has 0.76 items per base and the plan counts 1.04: 36.5 > 0.7336 * 30 - 4.3 = 17.7, so the stage runs in two or
# more passes, the later ones appending their items
@pytest.mark.parametrize("device", ["whole", "small"])
def test_cli_with_the_knob_writes_the_same_files_inside_its_budget(job, device, tmp_path):
    args, bases, want = job
    out = str(tmp_path / "on")
    env = {"MHX_S1_AGG_WIDE": "1"}
    if device == "small":
        env["MHX_FREE_BYTES"] = str(30 * bases)
    err = _core(gu.MHX_CORE, args, out, env=env)
    print("\n".join(line for line in err.splitlines() if "Memory plan" in line or "Device memory of" in line or "Stage 1 plan" in line))
    assert MARKER in err, err[-2000:]
    stages = _stages(err)
    assert [s[0] for s in stages] == ["stage 1", "stage 2"], stages
    if device == "small":
        assert stages[0][4] >= 2, stages
    _check_budget(stages)
    assert {"sdbg": canon.digest_sdbg(out), "counting": canon.digest_file(out + ".counting")} == want
