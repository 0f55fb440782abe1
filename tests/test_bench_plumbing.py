"""CPU: the evidence plumbing of bench.py (no GPU work): PMC traffic lookup, the committed profile files, and its options — a plain
run times its steps and nothing else, --full adds the figures beside the headline, --dump-outputs writes the outputs as floats."""
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_pmc_traffic_lookup_is_tied_to_the_kernel_sources(tmp_path, monkeypatch):
    """roofline.traffic comes from a committed PMC measurement only if that measurement was taken on the very kernel
    sources that are running (megahit_amd/buildid.py)"""
    import bench
    from megahit_amd.buildid import build_id, lib_id
    doc = {"build_id": build_id(), "lib_id": lib_id(),
           "kernels": {"k_radix_onesweep<3, 8, 3, SrcArray<3> >": {"hbm_bytes": 40000000000},
                       "k_radix_onesweep<3, 8, 3, S1Gen>": {"hbm_bytes": 25000000000},
                       "k_radix_onesweep<2, 8, 2, SrcArray<2> >": {"hbm_bytes": 2000000000},
                       "k_s1_stream<false, 4, 1024, 13>": {"hbm_bytes": 250000000},
                       "k_s1_stream<true, 4, 1024, 13>": {"hbm_bytes": 21000000000}}}
    p = str(tmp_path / "pmc.json")
    with open(p, "w") as f:
        json.dump(doc, f)
    traffic, src = bench.pmc_traffic("radix_scatter_12B", p)
    assert traffic == 40000000000 and "k_radix_onesweep<3" in src
    assert bench.pmc_traffic("radix_scatter_12B_gen", p)[0] == 25000000000
    assert bench.pmc_traffic("radix_scatter_8B", p)[0] == 2000000000
    assert bench.pmc_traffic("s1_groups", p)[0] == 21000000000
    doc["lib_id"] = "1" * 16  # another binary: accepted only if it was built from the current sources (not older than any of them)
    with open(p, "w") as f:
        json.dump(doc, f)
    monkeypatch.setattr(bench, "lib_built_from_current_sources", lambda: True)
    assert bench.pmc_traffic("radix_scatter_12B", p)[0] == 40000000000
    monkeypatch.setattr(bench, "lib_built_from_current_sources", lambda: False)
    traffic, why = bench.pmc_traffic("radix_scatter_12B", p)
    assert traffic is None and "another build of libmhx.so" in why
    doc["build_id"] = "0" * 16
    with open(p, "w") as f:
        json.dump(doc, f)
    traffic, why = bench.pmc_traffic("radix_scatter_12B", p)
    assert traffic is None and "other kernel sources" in why


def test_committed_bench_line_has_the_contract_fields():
    """the round's committed evidence is self-consistent: the bench line quotes the counter measurement of the build it ran on"""
    import glob
    lines = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench.json")))
    assert lines
    with open(lines[-1]) as f:
        d = json.loads(f.read())
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "parity_checked", "e2e"):
        assert key in d, key
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1 and d["roofline"]["peak"] == 8000.0
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-3
    assert d["cpu_baseline"]["kind"] == "reference" and d["cpu_baseline"]["cores"] >= 1
    assert "workload" in d["config"] and d["vs_baseline"] is None
    assert d["parity_checked"] is True and d["parity"]["digest"] == d["parity"]["reference_digest"]
    # the counter measurement the line quotes: the file of the same round, taken on the build the line ran on
    tag = os.path.basename(lines[-1])[:3]
    with open(os.path.join(ROOT, "profiles", tag + "_pmc_traffic.json")) as f:
        pmc = json.load(f)
    if d["roofline"]["traffic"] is not None:
        assert d["roofline"]["traffic"] in [v["hbm_bytes"] for v in pmc["kernels"].values()]
        assert d.get("build_id") in (None, pmc["build_id"])


def test_bench_with_several_gpus_launches_its_own_ranks():
    """`python bench.py --gpus N` the way `--gpus 1` is called, without a launcher (no WORLD_SIZE): the script becomes the launcher —
    torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1 — instead of exiting with "launch with torch.distributed.run"
    (VERDICT r4 weak #8).  No GPU here: every one of the N ranks gets as far as the check for one."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd="/tmp", env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)  # (the first `import torch` of a fresh container takes minutes)
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert p.returncode == 0 and p.stdout.strip().startswith("{")
        return
    assert p.returncode != 0
    assert "launch with torch.distributed.run" not in p.stderr
    started = p.stderr.count("bench.py needs a GPU") + p.stderr.count("this node shows")
    assert started == 2, p.stderr[-1500:]


class FakeSdbgEngine:
    """stands in for lib.Engine on a machine without a GPU: every step leaves the same small SdBG (3 of 65536 buckets filled,
    gaps of junk between them in the byte buffer) and counts the calls of the timed path"""
    def __init__(self, device=0, n_bytes=1000):
        from megahit_amd import canon, lib
        self.calls = {"s1": 0, "profile": 0}
        rng = np.random.default_rng(5)
        self.items = np.zeros(lib.NUM_BUCKETS, dtype=np.uint64)
        self.tips = np.zeros(lib.NUM_BUCKETS, dtype=np.uint64)
        self.large = np.zeros(lib.NUM_BUCKETS, dtype=np.uint64)
        self.off = np.zeros(lib.NUM_BUCKETS, dtype=np.uint64)
        o = 0
        for b, (ni, nt, nl) in zip((7, 300, 65535), ((n_bytes // 2, 2, 1), (4, 0, 0), (n_bytes, 1, 3))):
            self.items[b], self.tips[b], self.large[b], self.off[b] = ni, nt, nl, o
            o += canon.sdbg_bucket_nbytes(ni, nt, nl, 2) + 17  # 17 bytes nobody owns after every bucket
        self.data = rng.integers(0, 256, o, dtype=np.uint8)
        self.bufs = {lib.BUF_SDBG_BYTES: self.data, lib.BUF_BUCKET_COUNT: self.items, lib.BUF_BUCKET_TIPS: self.tips,
                     lib.BUF_BUCKET_LARGE: self.large, lib.BUF_BUCKET_OFFSET: self.off}

    def load_sequences(self, *a):
        pass

    def read2sdbg_s1(self, k, m):
        self.calls["s1"] += 1
        return types.SimpleNamespace(n_items=11, n_solid=5)

    def read2sdbg_s2(self, k, m):
        return types.SimpleNamespace(n_items=13, n_sdbg=int(self.items.sum()), n_tips=3, n_large=4, sdbg_bytes=self.data.size)

    def last_s1_plan(self):
        return "fake"

    def fetch(self, which, dtype):
        return self.bufs[which].view(dtype).copy()

    def synchronize(self):
        pass

    def profile(self, on):
        self.calls["profile"] += 1

    def profile_reset(self):
        pass

    def profile_get(self):
        return {"kernel": {"ms": 1.0, "launches": 2, "bytes": 1e6}}

    def close(self):
        pass


def test_bench_options_default_to_a_plain_run():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def _load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_sdbg_of_the_last_step_as_floats(tmp_path):
    """the bytes of every bucket (not what lies between them), the per-bucket tables and the totals: float32/float64, exact"""
    import bench
    from megahit_amd import canon
    eng = FakeSdbgEngine()
    res = (eng.read2sdbg_s1(21, 2), eng.read2sdbg_s2(21, 2))
    n = bench.dump_outputs(eng, "read2sdbg", res, str(tmp_path / "a"))
    got = _load_dump(str(tmp_path / "a"))
    assert set(got) == {"totals", "bucket_items", "bucket_tips", "bucket_large", "sdbg_bytes"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert n == sum(v.nbytes for v in got.values()) <= bench.DUMP_LIMIT_BYTES
    want = np.concatenate([eng.data[int(eng.off[b]):int(eng.off[b]) + canon.sdbg_bucket_nbytes(int(eng.items[b]), int(eng.tips[b]), int(eng.large[b]), 2)]
                           for b in (7, 300, 65535)])
    assert np.array_equal(got["sdbg_bytes"], want.astype(np.float32))
    assert np.array_equal(got["bucket_items"], eng.items.astype(np.float64))
    assert list(got["totals"]) == [11, 5, 13, int(eng.items.sum()), 3, 4, eng.data.size]


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    """an output too large to write whole: a seeded sample of fixed positions plus exact chunk sums over all of its bytes"""
    import bench
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 256)
    monkeypatch.setattr(bench, "DUMP_CHUNK", 1000)
    eng = FakeSdbgEngine(n_bytes=3000)
    res = (eng.read2sdbg_s1(21, 2), eng.read2sdbg_s2(21, 2))
    bench.dump_outputs(eng, "read2sdbg", res, str(tmp_path / "a"))
    bench.dump_outputs(eng, "read2sdbg", res, str(tmp_path / "b"))
    a, b = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))
    assert "sdbg_bytes" not in a and a["sdbg_bytes_sample"].shape == (256,) and a["sdbg_bytes_sample"].dtype == np.float32
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    compact = bench.sdbg_compact_bytes(eng)[0]
    sums = a["sdbg_bytes_chunk_sums"]
    assert sums.dtype == np.float64 and sums.shape == ((compact.size + 999) // 1000,)
    last = compact[(sums.size - 1) * 1000:]
    assert sums[-1] == sum(int(x) * (i % 251 + 1) for i, x in enumerate(last))
    eng.data[int(eng.off[300])] ^= 1  # one byte of the output changes: the chunk sums see it
    bench.dump_outputs(eng, "read2sdbg", res, str(tmp_path / "c"))
    assert not np.array_equal(_load_dump(str(tmp_path / "c"))["sdbg_bytes_chunk_sums"], sums)


def _run_bench(monkeypatch, capfd, argv, fake):
    """bench.main() end to end with the engine and the device stood in for; -> (JSON line, names of the extras that ran)"""
    import torch
    import bench
    from megahit_amd import lib
    ran = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(lib, "Engine", lambda device: fake)
    monkeypatch.setattr(bench, "make_reads", lambda n, r, w: np.zeros(4, dtype=np.uint32))
    for name, value in (("end_to_end", {"wall_s": 1.0}), ("cpu_baseline", {"value": 1.0}), ("copy_bandwidth", 5000.0),
                        ("output_parity", {"checked": True})):
        monkeypatch.setattr(bench, name, lambda *a, _n=name, _v=value, **k: ran.append(_n) or _v)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    saved = os.dup(1)
    try:
        bench.main()
    finally:
        os.dup2(saved, 1)
        os.close(saved)
    out = capfd.readouterr().out.strip().splitlines()
    assert len(out) == 1, out
    return json.loads(out[0]), ran


def test_plain_bench_run_times_its_steps_and_nothing_else(monkeypatch, capfd, tmp_path):
    fake = FakeSdbgEngine()
    d, ran = _run_bench(monkeypatch, capfd, ["--gpus", "1", "--steps", "4", "--warmup", "3", "--no-cpu-full",
                                             "--dump-outputs", str(tmp_path / "out")], fake)
    assert ran == [] and fake.calls["profile"] == 0
    assert fake.calls["s1"] == 3 + 4 and d["steps"] == 4 and d["warmup"] == 3
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["unit"] == "M edges/s" and d["higher_is_better"] is True and d["dtype"] == "u32" and d["ms_per_step"] > 0
    assert not {"roofline", "parity", "parity_checked", "cpu_baseline", "e2e"} & set(d)
    assert os.path.exists(str(tmp_path / "out" / "sdbg_bytes.npy"))


def test_full_bench_run_adds_the_figures_beside_the_headline(monkeypatch, capfd):
    fake = FakeSdbgEngine()
    d, ran = _run_bench(monkeypatch, capfd, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-full"], fake)
    assert sorted(ran) == ["copy_bandwidth", "cpu_baseline", "end_to_end", "output_parity"]
    assert fake.calls["s1"] == 3 and fake.calls["profile"] == 2
    assert d["roofline"]["kernel"] == "kernel" and d["parity_checked"] is True and d["e2e"] == {"wall_s": 1.0}
    assert d["cpu_baseline"]["value"] == 1.0
