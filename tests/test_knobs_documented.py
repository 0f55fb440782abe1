"""Every knob of the table (megahit_amd/csrc/mhx_options.h: mhx_set_option / MHX_<NAME> / mhx_tuning.conf) is described in
include/mhx.h or INTEGRATION.md — a caller of the C ABI meets no switch that only the source knows —, no source reads a knob
past the table, and where the description states a default as `name (integer)` it is the table's."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megahit_amd", "csrc")


def table():
    """name -> default (None: derived, the reading site supplies it)"""
    with open(os.path.join(CSRC, "mhx_options.h")) as fh:
        body = fh.read().split("#define MHX_OPTIONS(X, D)", 1)[1].split("namespace mhx", 1)[0]
    knobs = {}
    for name, dflt in re.findall(r"^\s*X\(([a-z0-9_]+),\s*([^)]+)\)", body, re.M):
        assert name not in knobs, name
        m = re.fullmatch(r"(\d+) << (\d+)", dflt)
        knobs[name] = int(m.group(1)) << int(m.group(2)) if m else int(dflt)
    for name in re.findall(r"^\s*D\(([a-z0-9_]+)\)", body, re.M):
        assert name not in knobs, name
        knobs[name] = None
    assert len(knobs) == len(re.findall(r"^\s*[XD]\(", body, re.M))  # (no line of the list escaped the two patterns)
    return knobs


def docs():
    with open(os.path.join(ROOT, "include", "mhx.h")) as fh:
        doc = fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        return doc + fh.read()


def test_every_knob_is_documented():
    names = set(table())
    doc = docs()
    assert len(names) > 50
    missing = sorted(n for n in names if n not in doc)
    assert not missing, missing


def test_no_source_reads_a_knob_by_a_string_literal():
    hits = []
    for f in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True):
        if f.endswith((".hip", ".h", ".cpp")):
            with open(f) as fh:
                hits += ["%s: %s" % (os.path.relpath(f, ROOT), m) for m in re.findall(r'\bopt\s*(?:<[^>]*>)?\s*\(\s*"[^"]*"', fh.read())]
    assert not hits, hits


def test_documented_defaults_are_the_tables():
    knobs = table()
    stated = {}
    for name, dflt in re.findall(r"\b([a-z][a-z0-9_]+) \((-?\d+)\)", docs()):
        if knobs.get(name) is not None:  # (a derived knob's default is a size of its reading site: the table has nothing to compare)
            stated.setdefault(name, set()).add(int(dflt))
    assert len(stated) >= 70  # (the form the descriptions use: a change of style must not empty the check)
    wrong = {n: (sorted(v), knobs[n]) for n, v in stated.items() if v != {knobs[n]}}
    assert not wrong, wrong
