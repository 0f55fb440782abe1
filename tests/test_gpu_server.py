"""GPU: the sub-programs through the resident server (`mhx_core --serve`, clients with MHX_SERVER): one process keeps the
handle and its device buffers across count -> seq2sdbg -> read2sdbg -> ... and every request still reproduces the
reference's digests (tests/golden/golden.json) — state of one request must not leak into the next."""
import os
import subprocess
import time

import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sock_dir():
    with gu.socket_dir() as d:
        yield d


@pytest.fixture(scope="module")
def server(tmp_path_factory, sock_dir):
    d = tmp_path_factory.mktemp("srv")
    sock = os.path.join(sock_dir, "mhx.sock")
    log = open(str(d / "server.log"), "w")
    p = subprocess.Popen([gu.MHX_CORE, "--serve", sock], stdout=subprocess.DEVNULL, stderr=log, env=dict(os.environ, MHX_SERVE_IDLE_S="60"))
    for _ in range(500):
        if os.path.exists(sock):
            break
        time.sleep(0.02)
    assert os.path.exists(sock)
    yield sock, p
    subprocess.run([gu.MHX_CORE, "--serve-stop", sock], timeout=60)
    try:
        p.wait(timeout=30)
    except subprocess.TimeoutExpired:
        p.kill()
    log.close()


def _pick():
    seen, out = set(), []
    for e in gu.cases():
        c = e["case"]
        key = (c["prog"], c.get("k"), c.get("mercy"), c.get("input"))
        if key in seen:
            continue
        seen.add(key)
        out.append(e)
    return out[:14]


@pytest.mark.parametrize("ent", _pick(), ids=gu.case_id)
def test_served_requests_reproduce_the_reference(ent, tmp_path, server, monkeypatch):
    sock, proc = server
    monkeypatch.setenv("MHX_SERVER", sock)
    got = gu.run_case(gu.MHX_CORE, ent, str(tmp_path))
    for key, want in ent.items():
        if key in ("case", "mercy_cand_kmsort"):
            continue
        assert got.get(key) == want, key
    assert proc.poll() is None, "the server died"


def test_the_work_really_ran_in_the_server(tmp_path, server, monkeypatch):
    sock, _proc = server
    ent = [e for e in gu.cases() if e["case"]["prog"] == "count"][0]
    c = ent["case"]
    env = dict(os.environ, MHX_SERVER=sock)
    p = subprocess.run([gu.MHX_CORE, "count", "-k", str(c["k"]), "-m", str(c["m"]), "--read_lib_file", os.path.join(gu.GOLD, c["lib"]),
                        "--output_prefix", str(tmp_path / "o"), "--host_mem", "2e9", "--num_cpu_threads", "3"], stderr=subprocess.PIPE, text=True, env=env)
    assert p.returncode == 0
    assert "server: totals since its start" in p.stderr


def test_under_the_references_name_the_server_is_the_default(tmp_path, monkeypatch, sock_dir):
    """megahit_core -> mhx_core (how an unmodified orchestrator finds us): no environment variable, and the first sub-program starts
    the resident server (one per user and device, in $XDG_RUNTIME_DIR), the second finds it; the outputs stay the reference's;
    a request whose chained-scan sort gives up (test hook) is run again with the classic passes inside the server; MHX_SERVER=off
    keeps the work in the calling process"""
    drop_in = os.path.join(os.path.dirname(gu.MHX_CORE), "megahit_core")
    if not os.path.exists(drop_in):
        os.symlink("mhx_core", drop_in)
    monkeypatch.delenv("MHX_SERVER", raising=False)
    rt = os.path.join(sock_dir, "rt")
    os.mkdir(rt)
    monkeypatch.setenv("XDG_RUNTIME_DIR", rt)
    monkeypatch.setenv("MHX_SERVE_IDLE_S", "60")
    sock = subprocess.run([gu.MHX_CORE, "--default-socket"], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    assert os.path.dirname(sock) == rt
    ents = [e for e in gu.cases() if e["case"]["k"] == 21 and e["case"].get("lib") == "hc" and not e["case"].get("input")][:3]
    try:
        for i, ent in enumerate(ents + ents[:1]):
            if i == len(ents):
                monkeypatch.setenv("MHX_TEST_SCAN_TIMEOUT_ONCE", "1")
            out = tmp_path / ("o%d" % i)
            out.mkdir()
            got = gu.run_case(drop_in, ent, str(out))
            for key, want in ent.items():
                if key in ("case", "mercy_cand_kmsort"):
                    continue
                assert got.get(key) == want, key
            assert os.path.exists(sock), "no server was started"
        monkeypatch.delenv("MHX_TEST_SCAN_TIMEOUT_ONCE")
        # the request ran in the server: the client's own log has no device line of its own
        c = ents[0]["case"]
        p = subprocess.run([drop_in, c["prog"], "-k", str(c["k"]), "-m", str(c["m"]), "--read_lib_file", os.path.join(gu.GOLD, c["lib"]),
                            "--output_prefix", str(tmp_path / "again"), "--host_mem", "2e9", "--num_cpu_threads", "3"], stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0 and "server: totals since its start" in p.stderr, p.stderr[-600:]
        monkeypatch.setenv("MHX_SERVER", "off")
        p = subprocess.run([drop_in, c["prog"], "-k", str(c["k"]), "-m", str(c["m"]), "--read_lib_file", os.path.join(gu.GOLD, c["lib"]),
                            "--output_prefix", str(tmp_path / "own"), "--host_mem", "2e9", "--num_cpu_threads", "3"], stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0 and "server: totals since its start" not in p.stderr, p.stderr[-600:]
    finally:
        subprocess.run([gu.MHX_CORE, "--serve-stop", sock], timeout=60)


def test_settings_of_one_request_do_not_stick_to_the_server(tmp_path, server):
    """the environment settings libmhx reads (MHX_S2_PER_OCCURRENCE, MHX_S1_MARK, the mhx_set_option knobs as MHX_<NAME>) are read per
    call, not cached in function-local statics: the same sub-program asked for with and without a setting, in both orders, by
    requests to one resident server, takes the path its own request names — seen from the stage-2 item count (per-occurrence items
    against aggregated ones) and the stage-1 plan line — and writes the same files every time"""
    import re
    from megahit_amd import canon
    sock, proc = server
    ent = [e for e in gu.cases() if e["case"]["prog"] == "read2sdbg" and e["case"]["k"] == 21 and not e["case"].get("mercy")][0]
    c = ent["case"]

    def call(tag, **extra):
        env = {k: v for k, v in os.environ.items() if k not in ("MHX_S2_PER_OCCURRENCE", "MHX_S1_MARK", "MHX_S1_STREAM", "MHX_SDBG_FAST")}
        env.update(MHX_SERVER=sock, **extra)
        out = str(tmp_path / tag)
        p = subprocess.run([gu.MHX_CORE, "read2sdbg", "-k", str(c["k"]), "-m", str(c["m"]), "--read_lib_file", os.path.join(gu.GOLD, c["lib"]),
                            "--output_prefix", out, "--host_mem", "2e9", "--num_cpu_threads", "3"], stderr=subprocess.PIPE, text=True, env=env)
        assert p.returncode == 0, p.stderr[-600:]
        items = int(re.search(r"Stage 2 done \((\d+) items\)", p.stderr).group(1))
        plan = re.search(r"Stage 1 plan: (.*)", p.stderr).group(1)
        return items, plan, canon.digest_sdbg(out)

    a_items, a_plan, a_dig = call("a")
    b_items, b_plan, b_dig = call("b", MHX_S2_PER_OCCURRENCE="1")
    c_items, c_plan, c_dig = call("c")
    d_items, d_plan, d_dig = call("d", MHX_S1_STREAM="0", MHX_SDBG_FAST="0")
    e_items, e_plan, e_dig = call("e")
    assert a_dig == b_dig == c_dig == d_dig == e_dig
    assert b_items > a_items and c_items == a_items == e_items  # per occurrence only while asked for
    assert "stream" in a_plan and "stream" not in d_plan and e_plan == a_plan == c_plan
    assert proc.poll() is None, "the server died"
