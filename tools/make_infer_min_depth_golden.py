"""Writes tests/golden/infer_min_depth.json: for a few synthetic libraries, what the reference's own `megahit_core assemble -t 1`
does on the SdBG of its own `read2sdbg` when NO positive `--min_depth` is given, so that sdbg_pruning::InferMinDepth decides it —
the digests of the eight output files (make_unitig_prune_golden.FILES), the counts parsed from its log, the string it logs after
"min depth set to" and the reference's own multiplicity histogram over the valid edges of the graph as loaded (the `mul` and
`invalid` sections of oracle/_ref/ref_sdbg_dump), as a sparse [value, count] list.  tests/test_infer_min_depth.py runs the host
function on those histograms; tests/test_gpu_infer_min_depth.py compares the device's histogram with them and mhx_core (its route's
opt-in variable at 2) with the files, counts and logged depth, without the reference.  Runs on the CPU:

    python tools/make_infer_min_depth_golden.py [--ref oracle/_ref/ref_megahit_core] [--dump oracle/_ref/ref_sdbg_dump]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_unitig_bubble_golden as mbg  # noqa: E402
import make_unitig_prune_golden as mpg  # noqa: E402

mcg = mpg.mcg
FILES = mpg.FILES
# route: the opt-in variable under which mhx_core serves the command line, at the value 2 (MHX_ASSEMBLE_PRUNE / MHX_ASSEMBLE_BUBBLE)
CASES = [  # name, library + graph, the assemble options behind `-s -o -t`
    dict(mcg.A, name="A-p2", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "2"]),
    # the boundary of `min_depth <= 0`
    dict(mcg.A, name="A-p1-final-depth0", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "1", "--is_final_round", "--min_depth", "0"]),
    dict(mcg.B, name="B-m1-p2", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "2"]),
    # what the orchestrator passes for `megahit --prune-level 3` without --prune-depth.  (This case and the next at 2 % errors: on A's
    # own 1 % the rounds leave the same contig whether the depth is the inferred 5.099 or the min count)
    dict(mcg.A, err=0.02, name="A-orchestrator-p3", route="BUBBLE",
         args=["--bubble_level", "2", "--prune_level", "3", "--careful_bubble", "--min_depth", "-1"] + mbg.ORCH),
    # no option at all: the sub-program's defaults (bubble level 2, prune level 2, --min_depth -1)
    dict(mcg.A, err=0.02, name="A-defaults", route="BUBBLE", args=[]),
    # low coverage: the counts fall from multiplicity 1 on, FirstLocalMinimum finds its minimum at the largest value and returns 0
    dict(mcg.B, pairs=300, name="B-lowcov-firstmin0", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "2"]),
    # 400 x: more than 8 % of the multiplicities are above 254 and the loader keeps full_mul (at A's 1 % errors the erroneous edges seen
    # twice outnumber the genome's so far that only 5 % are: half the error rate)
    dict(mcg.A, G=2000, err=0.005, name="A-highcov-fullmul", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "2"]),
    dict(mcg.E, name="E-k63-mercy", route="PRUNE", args=["--bubble_level", "0", "--prune_level", "2"]),
]
LIBRARY = ("kind", "G", "pairs", "err", "seed", "read_len", "frag", "k", "m", "mercy")


def parse_log(route, text):
    """the counts of the route's own golden tool plus the string logged after "min depth set to" (None: no such line)"""
    out = mpg.parse_log(text) if route == "PRUNE" else mbg.parse_log(text)
    m = re.search(r"min depth set to (\S+)", text)
    out["min_depth"] = m.group(1) if m else None
    out["unconverged"] = "Cannot detect min depth: unconverged" in text
    return out


def read_dump(path):
    """the sections of a ref_sdbg_dump file (oracle/ref_sdbg_dump.cpp): name -> raw bytes, element size"""
    out = {}
    with open(path, "rb") as f:
        data = f.read()
    pos = 0
    while pos < len(data):
        name = data[pos:pos + 32].split(b"\0")[0].decode()
        elem, n = (int(x) for x in np.frombuffer(data, dtype=np.uint64, count=2, offset=pos + 32))
        out[name] = (data[pos + 48:pos + 48 + elem * n], elem)
        pos += 48 + elem * n
    return out


def reference_histogram(dump_exe, g, d):
    """-> (sparse [value, count] list over the valid edges of the graph as the reference loads it, n, large multiplicities, full_mul)"""
    path = os.path.join(d, "dump.bin")
    subprocess.run([dump_exe, g, path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = read_dump(path)
    meta = np.frombuffer(s["meta"][0], dtype=np.uint64)
    n = int(meta[0])
    mul = np.frombuffer(s["mul"][0], dtype=np.uint16)
    inv = np.unpackbits(np.frombuffer(s["invalid"][0], dtype=np.uint8), bitorder="little")[:n].astype(bool)
    h = np.bincount(mul[~inv], minlength=65536)
    return [[int(v), int(h[v])] for v in np.nonzero(h)[0]], n, int(meta[2]), int(meta[5])


def first_local_minimum(sparse):
    """Histgram::FirstLocalMinimum on a sparse ascending [value, count] list"""
    best, rising = 0, 0
    for i, (_, cnt) in enumerate(sparse):
        if cnt <= sparse[best][1]:
            best, rising = i, 0
        else:
            rising += 1
            if rising >= 4:
                break
    return 0 if best == len(sparse) - 1 else sparse[best][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "ref_megahit_core"))
    ap.add_argument("--dump", default=os.path.join(ROOT, "oracle", "_ref", "ref_sdbg_dump"))
    a = ap.parse_args()
    cases = []
    for c in CASES:
        with tempfile.TemporaryDirectory() as d:
            g = mpg.build_graph(a.ref, c, d)
            out = os.path.join(d, "ref")
            log = parse_log(c["route"], mpg.run_assemble(a.ref, g, out, c["args"]))
            hist, n, n_large, full_mul = reference_histogram(a.dump, g, d)
            rec = dict(c, digests=mpg.digests(out), log=log, n_items=n, n_large=n_large, full_mul=full_mul, hist=hist)
            # the same options with the graph's min count as an explicit depth: what the inference decided
            given = os.path.join(d, "given")
            args = [x for i, x in enumerate(c["args"]) if x != "--min_depth" and (i == 0 or c["args"][i - 1] != "--min_depth")]
            mpg.run_assemble(a.ref, g, given, args + ["--min_depth", str(c["m"])])
            rec["contigs_differ_from_min_depth_m"] = mpg.digests(given)[".contigs.fa"] != rec["digests"][".contigs.fa"]
        assert sorted(rec["digests"]) == sorted(FILES), (c["name"], sorted(rec["digests"]))
        # a case that shows nothing gets another seed or coverage and is not kept
        assert log["min_depth"] is not None and not log["unconverged"], (c["name"], log)
        if c["name"] == "B-lowcov-firstmin0":
            assert first_local_minimum(hist) == 0, (c["name"], hist[:8])
        else:
            assert first_local_minimum(hist) > 0, (c["name"], hist[:8])
        if c["name"] == "A-highcov-fullmul":
            assert n_large >= 0.08 * n and full_mul == 1, (c["name"], n, n_large, full_mul)
        else:
            assert full_mul == 0, (c["name"], n, n_large)
        cases.append(rec)
        print(c["name"], log, n, n_large, rec["contigs_differ_from_min_depth_m"], file=sys.stderr)
    assert any(float(c["log"]["min_depth"]) != int(float(c["log"]["min_depth"])) for c in cases)
    assert sum(c["contigs_differ_from_min_depth_m"] for c in cases) >= 3
    with open(os.path.join(ROOT, "tests", "golden", "infer_min_depth.json"), "w") as f:
        # one case per line: the digests and the histogram are most of the file
        f.write('{"what": "reference megahit_core assemble -t 1 without a positive --min_depth (InferMinDepth) on its own read2sdbg graph; '
                'hist = its EdgeMultiplicity histogram over the valid edges as loaded",\n'
                ' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases) + "\n ]}\n")


if __name__ == "__main__":
    main()
