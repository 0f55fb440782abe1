"""GPU: `mhx_core --gpus N count` on super-k-mer records exchanged by bin (MHX_COUNT_SKM_DIST=1; comm.hip dist_count_skm) against the golden
digests, and the same driver with the ranks as separate processes over the hosted transport (the machinery of test_gpu_multiprocess.py)."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import test_gpu_multiprocess as tgm
from megahit_amd import canon

pytestmark = pytest.mark.gpu

ENV = dict(MHX_COUNT_SKM_DIST="1", MHX_S1_SKM="2", MHX_S1_SKM_MAX_BIN=str(1 << 30), MHX_S1_VAR_MIN_FILL="5")
CASES = [e for e in gu.cases() if e["case"]["prog"] == "count" and e["case"]["k"] == 21 and e["case"]["m"] == 2 and e["case"]["lib"] in ("r3", "hc", "rag")]


def set_env(monkeypatch, gpus):
    monkeypatch.setenv("MHX_NUM_GPUS", str(gpus))
    monkeypatch.setenv("MHX_GPU_MAP", ",".join("0" for _ in range(gpus)))
    for name, v in ENV.items():
        monkeypatch.setenv(name, v)


def test_the_three_golden_cases_are_there():
    assert sorted(e["case"]["lib"] for e in CASES) == ["hc", "r3", "rag"]


@pytest.mark.parametrize("ent", CASES, ids=gu.case_id)
@pytest.mark.parametrize("gpus", [4, 8])
def test_cli_count_reproduces_reference_on_the_bin_exchange(ent, gpus, tmp_path, monkeypatch):
    """every golden key through golden_util.run_case, whose calls are made to keep what the program logs: the plan line names the route"""
    set_env(monkeypatch, gpus)
    logs = []
    real_run = subprocess.run

    def run_keeping_stderr(args, **kw):
        kw["stderr"] = subprocess.PIPE
        p = real_run(args, **kw)
        logs.append(p.stderr.decode(errors="replace") if isinstance(p.stderr, bytes) else (p.stderr or ""))
        return p

    monkeypatch.setattr(gu.subprocess, "run", run_keeping_stderr)
    got = gu.run_case(gu.MHX_CORE, ent, str(tmp_path))
    monkeypatch.setattr(gu.subprocess, "run", real_run)
    for key, want in ent.items():
        if key == "case":
            continue
        assert got.get(key) == want, key
    assert logs and all("exchanged by bin" in text for text in logs), logs[-1][-2000:]


def test_cli_eight_gpus_on_five_reads(tmp_path, monkeypatch):
    """five reads over eight ranks, three of them without a read: whichever route the ranks agree on, the edges are oracle_core's"""
    from megahit_amd import synth
    d = str(tmp_path)
    genome = np.random.default_rng(41).integers(0, 4, size=300, dtype=np.uint8)
    reads = [genome[o:o + 100].copy() for o in (0, 40, 80, 120, 160)]
    synth.write_fasta(os.path.join(d, "r.fa"), reads)
    with open(os.path.join(d, "lib"), "w") as f:
        f.write("five reads\nse %s\n" % os.path.join(d, "r.fa"))
    lib_ = os.path.join(d, "five")
    subprocess.run([gu.MHX_CORE, "buildlib", os.path.join(d, "lib"), lib_], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   env=dict(os.environ, MHX_BUILDLIB_HOST="1"), timeout=120)
    args = ["count", "-k", "21", "-m", "2", "--read_lib_file", lib_, "--host_mem", "2e9", "--num_cpu_threads", "3"]
    subprocess.run([gu.ORACLE_CORE] + args + ["--output_prefix", os.path.join(d, "want")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=120)
    set_env(monkeypatch, 8)
    p = subprocess.run([gu.MHX_CORE] + args + ["--output_prefix", os.path.join(d, "got")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert canon.canonical_edges(os.path.join(d, "want"))[1].shape[0] > 0
    assert canon.digest_edges(os.path.join(d, "got")) == canon.digest_edges(os.path.join(d, "want"))


def _count_worker(rank, world, port, mode, k, m, opts, q):
    """test_gpu_multiprocess._worker's count job, with the plan line in what it reports (the knobs come from the environment)"""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle_binding as ob
    from dist_inputs import reads_of
    from megahit_amd import lib
    e = lib.Engine(0)
    pkg = ob.Package(reads_of(100 + rank, n_pairs=600), reverse=True)
    e.load_sequences(pkg.words(), pkg.n_seqs, 0, pkg.start())
    cm = lib.Comm.hosted(e, dist, rank, world)
    cm.setup(3, k, m)
    cm.count(k, m)
    out = {"rank": rank, "edges": e.fetch(lib.BUF_EDGES, np.uint32), "hist": e.fetch(lib.BUF_MUL_HIST, np.int64),
           "first": e.fetch(lib.BUF_FIRST_0_OUT, np.uint32), "last": e.fetch(lib.BUF_LAST_0_IN, np.uint32),
           "items": e.fetch(lib.BUF_BUCKET_COUNT, np.uint64), "plan": e.last_s1_plan()}
    q.put(out)
    dist.barrier()
    cm.close()
    e.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_count_rank_processes_on_the_bin_exchange(world, monkeypatch):
    """rank processes (at most four with the GPU open besides this one), the bytes moved by torch.distributed over gloo"""
    import oracle_binding as ob
    from dist_inputs import reads_of
    k, m = 21, 2
    for name, v in ENV.items():
        monkeypatch.setenv(name, v)
    monkeypatch.setattr(tgm, "_worker", _count_worker)
    outs = tgm.run_world(world, "count", k, m)
    assert all(o["plan"].startswith("count: super-k-mers") and "exchanged by bin" in o["plan"] for o in outs), [o["plan"] for o in outs]
    want = ob.count(ob.Package(sum((reads_of(100 + r, n_pairs=600) for r in range(world)), []), reverse=True), k, m)
    assert np.array_equal(np.concatenate([o["edges"] for o in outs]).reshape(-1, want["wpe"]), want["edges"])
    assert np.array_equal(sum(o["items"] for o in outs), want["bucket_count"])
    assert np.array_equal(sum(o["hist"] for o in outs), want["hist"])
    assert np.array_equal(np.concatenate([o["first"] for o in outs]), want["first_0_out"])
    assert np.array_equal(np.concatenate([o["last"] for o in outs]), want["last_0_in"])
